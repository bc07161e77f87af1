"""numpy restatement of the point-pair-feature definition of include/pose_refine.h ("hypotheses from the scene"): frames, features, keys, the
model's buckets, a reference's accumulator, peaks in the header's total order, the float64 pose of a peak, the sampler's lattice, and the
hypothesis list.  float32 arithmetic in the header's operand order (numpy rounds every float32 operation once, sqrt and division correctly);
it shares no code with the library and reads the bin-edge and bin-centre tables from the descriptor, never recomputing them.
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def tables(pp):
    """The descriptor's fields as numpy values."""
    return dict(inv=F(pp.inv_dist_step), n_dist=int(pp.n_dist), A=int(pp.n_angle), n_alpha=int(pp.n_alpha), n_keys=int(pp.n_keys),
                cos_edge=np.array(pp.cos_edge[:], F), alpha_edge=np.array(pp.alpha_edge[:], F),
                alpha_cos=np.array(pp.alpha_cos[:], np.float64), alpha_sin=np.array(pp.alpha_sin[:], np.float64))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def good_len(v):
    return (v > 0) & (v <= FLT_MAX)


def axis_of(n):
    """The coordinate axis of the smallest |component|, the lowest index on a tie."""
    a = np.abs(np.asarray(n, F))
    if a[0] <= a[1] and a[0] <= a[2]:
        return 0
    return 1 if a[1] <= a[2] else 2


def frame(n):
    """(u, v) float32[3] each of an oriented point's normal, or None."""
    n = np.asarray(n, F)
    e = axis_of(n)
    z = F(0)
    w = [np.array([z, -n[2], n[1]], F), np.array([n[2], z, -n[0]], F), np.array([-n[1], n[0], z], F)][e]
    with np.errstate(all="ignore"):
        l = np.sqrt(dot3(w, w))
        if not good_len(l):
            return None
        u = (w / l).astype(F)
    v = np.array([n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]], F)
    return u, v


def edge_bin(edge, n, c):
    """The number of k in 1 .. n-1 with c <= edge[k], for an array of c."""
    return (np.asarray(c, F)[:, None] <= edge[None, 1:n]).sum(1).astype(np.int64)


def pairs(tb, pr, nr, P, N):
    """Reference (pr, nr) against all points (P, N): (ok bool[n], key int64[n], c float32[n], s float32[n])."""
    P, N, pr, nr = np.asarray(P, F), np.asarray(N, F), np.asarray(pr, F), np.asarray(nr, F)
    n = len(P)
    fr = frame(nr)
    if fr is None:
        return np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, F), np.zeros(n, F)
    u, v = fr
    with np.errstate(all="ignore"):
        d = (P - pr[None]).astype(F)
        L = np.sqrt(dot3(d, d))
        t = L * tb["inv"]
        c1 = dot3(nr[None], d) / L
        c2 = dot3(N, d) / L
        c3 = dot3(nr[None], N)
        y, z = dot3(d, u[None]), dot3(d, v[None])
        r = np.sqrt(y * y + z * z)
        ok = good_len(L) & (t < F(tb["n_dist"])) & np.isfinite(c1) & np.isfinite(c2) & np.isfinite(c3) & good_len(r)
        c, s = y / r, z / r
    A = tb["A"]
    bd = np.where(ok, t, 0).astype(np.int64)
    key = ((bd * A + edge_bin(tb["cos_edge"], A, c1)) * A + edge_bin(tb["cos_edge"], A, c2)) * A + edge_bin(tb["cos_edge"], A, c3)
    assert c.dtype == F and s.dtype == F and t.dtype == F
    return ok, np.where(ok, key, 0), c, s


def alpha_bins(tb, cs, ss, cm, sm):
    """Bins of (scene angle) - (model angle) for arrays of unit vectors; -1: no vote."""
    with np.errstate(all="ignore"):
        ca = cs * cm + ss * sm
        sa = ss * cm - cs * sm
        q = np.sqrt(ca * ca + sa * sa)
        ok = good_len(q)
        cn = ca / q
    assert cn.dtype == F
    na = tb["n_alpha"]
    h = edge_bin(tb["alpha_edge"], na // 2, cn)
    return np.where(ok, np.where(sa >= 0, h, na - 1 - h), -1)


def model_table(tb, pts, nrm):
    """The model's buckets: offsets int64[n_keys + 1] and the entries sorted by (key, pair): dict(key, pair, c, s)."""
    n = len(pts)
    K, PR, Cc, Ss = [], [], [], []
    for r in range(n):
        ok, key, c, s = pairs(tb, pts[r], nrm[r], pts, nrm)
        ok[r] = False
        i = np.flatnonzero(ok)
        K.append(key[i]); PR.append((r << 16) | i); Cc.append(c[i]); Ss.append(s[i])
    K, PR, Cc, Ss = np.concatenate(K), np.concatenate(PR), np.concatenate(Cc), np.concatenate(Ss)
    o = np.lexsort((PR, K))
    offsets = np.zeros(tb["n_keys"] + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(K, minlength=tb["n_keys"]))
    return offsets, dict(key=K[o], pair=PR[o].astype(np.uint32), c=Cc[o], s=Ss[o])


def accumulator(tb, offsets, ent, n_model, spts, snrm, ref):
    """(acc int64[n_model, n_alpha], n_pairs) of scene reference `ref`."""
    ok, key, c, s = pairs(tb, spts[ref], snrm[ref], spts, snrm)
    i = np.flatnonzero(ok)
    na = tb["n_alpha"]
    acc = np.zeros(n_model * na, np.int64)
    lo, cnt = offsets[key[i]], offsets[key[i] + 1] - offsets[key[i]]
    tot = int(cnt.sum())
    if tot:
        start = np.cumsum(cnt) - cnt
        e = np.repeat(lo, cnt) + (np.arange(tot) - np.repeat(start, cnt))
        b = alpha_bins(tb, np.repeat(c[i], cnt), np.repeat(s[i], cnt), ent["c"][e], ent["s"][e])
        m = (ent["pair"][e] >> 16).astype(np.int64)
        good = b >= 0
        acc += np.bincount(m[good] * na + b[good], minlength=n_model * na)
    return acc.reshape(n_model, na), len(i)


def peaks(acc, n_peaks):
    """The first n_peaks cells in the order (votes descending, cell ascending) among those with votes: [(votes, model_ref, alpha_bin)]."""
    flat = acc.reshape(-1)
    o = np.argsort(-flat, kind="stable")[:n_peaks]
    return [(int(flat[c]), int(c // acc.shape[1]), int(c % acc.shape[1])) for c in o if flat[c] > 0]


def frame64(n):
    """Rows (nh, u, v) in float64 from a float32 normal, the header's pose frame."""
    n32 = np.asarray(n, F)
    x, y, z = (float(v) for v in n32)
    ln = np.sqrt((x * x + y * y) + z * z)
    h = (x / ln, y / ln, z / ln)
    e = axis_of(n32)
    w = [(0.0, -h[2], h[1]), (h[2], 0.0, -h[0]), (-h[1], h[0], 0.0)][e]
    lw = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    u = (w[0] / lw, w[1] / lw, w[2] / lw)
    v = (h[1] * u[2] - h[2] * u[1], h[2] * u[0] - h[0] * u[2], h[0] * u[1] - h[1] * u[0])
    return (h, u, v)


def peak_pose(tb, pm, nm, ps, ns, b, rounded=True):
    """The pose of a peak: float64 in the header's operand order, rounded to float32 once (or left in float64)."""
    Bm, Bs = frame64(nm), frame64(ns)
    c, s = float(tb["alpha_cos"][b]), float(tb["alpha_sin"][b])
    M = [[Bm[0][j] for j in range(3)], [c * Bm[1][j] - s * Bm[2][j] for j in range(3)], [s * Bm[1][j] + c * Bm[2][j] for j in range(3)]]
    p = [float(v) for v in np.asarray(pm, F)]
    q = [float(v) for v in np.asarray(ps, F)]
    T = np.zeros((4, 4), np.float64)
    for i in range(3):
        R = [(Bs[0][i] * M[0][j] + Bs[1][i] * M[1][j]) + Bs[2][i] * M[2][j] for j in range(3)]
        T[i, :3] = R
        T[i, 3] = q[i] - ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2])
    T[3, 3] = 1.0
    return T.astype(F) if rounded else T


def lattice(tri, step):
    """The sampler's lattice points of one triangle, float32[n, 3] in its order (i outer), or an empty array for a degenerate one."""
    a = np.asarray(tri, F).astype(np.float64)
    e1, e2 = a[1] - a[0], a[2] - a[0]
    nrm = np.cross(e1, e2)
    if not np.linalg.norm(nrm) > 0:
        return np.zeros((0, 3), F)
    N = max(1, int(np.ceil(max(np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(e2 - e1)) / float(step))))
    ij = np.array([(i, j) for i in range(N + 1) for j in range(N + 1 - i)], np.float64)
    return ((a[0][None] + (ij[:, :1] / N) * e1[None]) + (ij[:, 1:] / N) * e2[None]).astype(F)


def scene_points(pcd, normal, width, height, stride):
    """pr_ppf_scene_points_dev: (points float32[n, 3] in mm, normals float32[n, 3]) from dense metre arrays, row-major."""
    p = np.asarray(pcd, F).reshape(height, width, 3)[::stride, ::stride].reshape(-1, 3)
    n = np.asarray(normal, F).reshape(height, width, 3)[::stride, ::stride].reshape(-1, 3)
    keep = (n != 0).any(1) & (p[:, 2] > 0)
    return (p[keep] * F(1000.0)).astype(F), n[keep].copy()


def max_disp(Ta, Tb, pts):
    """Largest displacement of pts (float64) between two poses, mm."""
    d = (np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64))[:3]
    return float(np.sqrt(((pts @ d[:, :3].T + d[:, 3]) ** 2).sum(1).max()))


def hypotheses(tb, mpts, mnrm, spts, snrm, ref_stride, merge_mm, n_peaks=1):
    """api.generate_hypotheses restated: (poses float32[n, 4, 4], vote sums) in hand-on order, duplicates merged greedily by the largest
    displacement of the model points (float64 here, the device's float32 records there)."""
    offsets, ent = model_table(tb, mpts, mnrm)
    votes, poses = [], []
    for ref in range(0, len(spts), ref_stride):
        acc, _ = accumulator(tb, offsets, ent, len(mpts), spts, snrm, ref)
        pk = peaks(acc, n_peaks)
        for k in range(n_peaks):
            if k < len(pk):
                votes.append(pk[k][0]); poses.append(peak_pose(tb, mpts[pk[k][1]], mnrm[pk[k][1]], spts[ref], snrm[ref], pk[k][2]))
    votes, poses = np.array(votes, np.int64), np.array(poses, F).reshape(-1, 4, 4)
    order = np.argsort(-votes, kind="stable")
    P64 = np.asarray(mpts, np.float64)
    kept, total = [], np.zeros(len(votes), np.int64)
    for i in order:
        for j in kept:
            if max_disp(poses[i], poses[j], P64) <= merge_mm:
                total[j] += votes[i]
                break
        else:
            kept.append(i); total[i] += votes[i]
    kept = np.array(kept, np.int64)
    kept = kept[np.argsort(-total[kept], kind="stable")]
    return poses[kept], total[kept]
