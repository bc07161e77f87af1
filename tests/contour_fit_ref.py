"""Plain float64 reference of contour alignment (pr_scene_edge_nearest_dev, pr_contour_information, pr_info_combine, pr_info_eig, pr_info_step;
include/pose_refine.h): numpy in the header's order of operations over depth images rendered by the oracle, no code shared with the library.

  nearest_brute / nearest_separable   the nearest-edge map by exhaustive search of every window, and by a row pass and a column pass
  centers                             c_i = pose_i applied to the model centre, / 1000, rounded to float32
  fit_record                          classes, sum_d2 and the 30 sums of one render (math.fsum per component, the absolute sums beside them)
  combine / jacobi / step             the host-only calls
  refine                              the loop of api.refine_contours over callables
  plate_case                          a two-triangle plate in front of a wall: the surface leaves three motions free, the silhouette pins them

numpy evaluates elementwise IEEE operations without contraction, so each term equals the kernel's bit for bit and only the order of the additions
differs."""
from __future__ import annotations

import math

import numpy as np

import info_ref as I
from contour_ref import _drawn_window, edges
from pose_refine_amd import api

F32, F64 = np.float32, np.float64
NONE = 0xFFFFFFFF
FIT_FIELDS = ("contour", "used", "occluded", "miss", "sum_d2")
_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


# ---- the nearest scene edge pixel ----------------------------------------------------------------------------------------------------------------
def nearest_brute(e, radius):
    """The definition: per pixel, every edge pixel of its window, the least (dx^2 + dy^2, ey, ex)."""
    e = np.asarray(e, bool)
    h, w = e.shape
    out = np.full((h, w), NONE, np.uint32)
    for y in range(h):
        for x in range(w):
            y0, x0 = max(y - radius, 0), max(x - radius, 0)
            ys, xs = np.nonzero(e[y0:y + radius + 1, x0:x + radius + 1])
            if len(ys):
                ys, xs = ys + y0, xs + x0
                k = min(zip(((xs - x) ** 2 + (ys - y) ** 2).tolist(), ys.tolist(), xs.tolist()))
                out[y, x] = (k[1] << 16) | k[2]
    return out


def nearest_separable(e, radius):
    """The same by a row pass (nearest edge of the row within the radius, the left one on a tie) and a column pass over the 2 radius + 1 rows in
    ascending order, a later row winning only with a strictly smaller distance."""
    e = np.asarray(e, bool)
    h, w = e.shape
    xs = np.arange(w, dtype=np.int64)[None, :]
    big = 1 << 20
    left = np.maximum.accumulate(np.where(e, xs, -big), axis=1)
    right = np.minimum.accumulate(np.where(e, xs, big)[:, ::-1], axis=1)[:, ::-1]
    dl, dr = xs - left, right - xs
    off = np.where(dl <= dr, -dl, dr)
    has = np.minimum(dl, dr) <= radius
    best_d2 = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    out = np.full((h, w), NONE, np.int64)
    for dy in range(-radius, radius + 1):
        lo, hi = max(0, -dy), min(h, h - dy)                        # rows y with 0 <= y + dy < h
        if lo >= hi:
            continue
        src = slice(lo + dy, hi + dy)
        d2 = np.where(has[src], off[src] ** 2 + dy * dy, np.iinfo(np.int64).max)
        better = d2 < best_d2[lo:hi]
        ey = np.broadcast_to(np.arange(lo + dy, hi + dy, dtype=np.int64)[:, None], d2.shape)
        word = (ey << 16) | (xs + off[src])
        best_d2[lo:hi] = np.where(better, d2, best_d2[lo:hi])
        out[lo:hi] = np.where(better, word, out[lo:hi])
    return out.astype(np.uint32)


def nearest_ref(scene, jump, radius):
    """pr_scene_edge_nearest_dev: (H, W) uint32."""
    return nearest_separable(edges(scene, jump), radius)


# ---- the records of one render -------------------------------------------------------------------------------------------------------------------
def centers(poses, center_model):
    """float32[P, 3]: rows 0..2 of each pose applied to the centre in float64 (((m0 x + m1 y) + m2 z) + m3), / 1000.0, rounded."""
    M = np.asarray(poses, F32).reshape(-1, 4, 4).astype(F64)
    cm = np.asarray(center_model, F32).astype(F64)
    v = ((M[:, :3, 0] * cm[0] + M[:, :3, 1] * cm[1]) + M[:, :3, 2] * cm[2]) + M[:, :3, 3]
    return (v / 1000.0).astype(F32)


def fit_terms(img, scene, nearest, tau, jump, K, c, rho, origin=(0, 0)):
    """img: one render (the frame, or the ROI window whose frame position is `origin` = (x, y)); scene, nearest: the same pixels of the frame.
    Returns (counts dict, (2 * used, 30) float64 terms in pr_pose_info's column order)."""
    counts = dict.fromkeys(FIT_FIELDS, 0)
    win = _drawn_window(np.asarray(img))
    if win is None:
        return counts, np.zeros((0, I.N_SUMS), F64)
    r, s, N = np.asarray(img)[win].astype(np.int64), np.asarray(scene)[win].astype(np.int64), np.asarray(nearest)[win].astype(np.int64)
    e = edges(r, jump)
    occ = e & (s > 0) & (r - s > tau)
    used = e & ~occ & (N != NONE)
    ys, xs = np.nonzero(used)
    x = xs + win[1].start + origin[0]
    y = ys + win[0].start + origin[1]
    ex, ey = N[used] & 0xFFFF, N[used] >> 16
    counts.update(contour=int(e.sum()), used=int(used.sum()), occluded=int(occ.sum()), miss=int((e & ~occ & (N == NONE)).sum()),
                  sum_d2=int(((ex - x) ** 2 + (ey - y) ** 2).sum()))
    k = np.asarray(K, F32).reshape(-1).astype(F64)
    fx, cx, fy, cy = k[0], k[2], k[4], k[5]
    cc, rho = np.asarray(c, F32).astype(F64), F64(F32(rho))
    Z = r[used].astype(F64) / 1000.0
    ux, uy = x.astype(F64) - cx, y.astype(F64) - cy
    q = np.stack([ux * Z / fx - cc[0], uy * Z / fy - cc[1], Z - cc[2]], 1)
    one, zero = np.ones_like(Z), np.zeros_like(Z)
    rows = [(np.stack([one, zero, -(ux / fx)], 1), (ex - x).astype(F64) * Z / fx), (np.stack([zero, one, -(uy / fy)], 1), (ey - y).astype(F64) * Z / fy)]
    out = np.zeros((2 * len(Z), I.N_SUMS), F64)
    for half, (n, res) in enumerate(rows):
        J = np.empty((len(Z), 6), F64)
        J[:, 0] = (q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1]) / rho
        J[:, 1] = (q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2]) / rho
        J[:, 2] = (q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0]) / rho
        J[:, 3:] = n
        t = out[half::2]
        for col, (a, b) in enumerate(_UPPER):
            t[:, col] = J[:, a] * J[:, b]
        for a in range(6):
            t[:, 21 + a] = J[:, a] * res
        t[:, 27] = 1.0
        t[:, 28] = res * res
        t[:, 29] = res * res
    return counts, out


def fit_record(img, scene, nearest, tau, jump, K, c, rho, origin=(0, 0)):
    counts, t = fit_terms(img, scene, nearest, tau, jump, K, c, rho, origin)
    total, absum = I.sums(t)
    return dict(counts, sums=total, abs=absum)


def fit_records(renders, scene, nearest, tau, jump, K, cs, rho, roi=(0, 0, 0, 0)):
    """One fit_record per render; renders as oracle_lib.render returns them (with a ROI: the window's pixels)."""
    scene, nearest, origin = np.asarray(scene), np.asarray(nearest), (0, 0)
    if roi[2] > 0 and roi[3] > 0:
        x, y, w, h = roi
        scene, nearest, origin = scene[y:y + h, x:x + w], nearest[y:y + h, x:x + w], (x, y)
    return [fit_record(img, scene, nearest, tau, jump, K, cs[i], rho, origin) for i, img in enumerate(renders)]


def fit_bound(used, absum):
    """|device sum - fsum| <= (2 used + 16) * 2^-52 * sum |term|: info_ref.sum_bound with two terms per used pixel."""
    return I.sum_bound(2 * used, absum)


def info_of(rec, c, rho):
    """A POSE_INFO record from a reference record (counts and sums) -- what the host-only calls take."""
    o = np.zeros(1, api._lib.POSE_INFO)[0]
    o["n_points"], o["n_valid"] = rec.get("contour", rec.get("n_points", 0)), rec.get("used", rec.get("n_valid", 0))
    o["n_zero_weight"] = rec.get("n_zero_weight", 0)
    o["c"], o["rho"] = np.asarray(c, F32), F32(rho)
    o["H"], o["g"] = rec["sums"][:21], rec["sums"][21:27]
    o["sum_w"], o["sum_wr2"], o["sum_r2"] = rec["sums"][27], rec["sums"][28], rec["sums"][29]
    return o


# ---- the host-only calls -------------------------------------------------------------------------------------------------------------------------
def combine(a, wa, b, wb):
    """pr_info_combine on two POSE_INFO records."""
    assert np.asarray(a["c"]).tobytes() == np.asarray(b["c"]).tobytes() and F32(a["rho"]).tobytes() == F32(b["rho"]).tobytes()
    o = np.array(a).copy()
    for f in ("H", "g", "sum_w", "sum_wr2"):
        o[f] = F64(wa) * np.asarray(a[f], F64) + F64(wb) * np.asarray(b[f], F64)
    o["sum_r2"] = F64(a["sum_r2"]) + F64(b["sum_r2"])
    for f in ("n_points", "n_valid", "n_zero_weight"):
        o[f] = int(a[f]) + int(b[f])
    return o


def jacobi(h21, max_sweeps=16):
    """The header's cyclic Jacobi in Python floats (IEEE doubles, every operation rounded on its own): (lambda[6], V[6, 6], sweeps)."""
    A = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(_UPPER):
        A[i][j] = A[j][i] = float(h21[k])
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    sweeps = 0
    while sweeps < max_sweeps:
        off = max(abs(A[i][j]) for i in range(6) for j in range(i + 1, 6))
        diag = max(abs(A[i][i]) for i in range(6))
        if off <= 2.0 ** -56 * diag:
            break
        for p in range(5):
            for q in range(p + 1, 6):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] -= t * apq
                A[q][q] += t * apq
                A[p][q] = A[q][p] = 0.0
                for k in range(6):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                for k in range(6):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
        sweeps += 1
    lam, V = np.array([A[i][i] for i in range(6)], F64), np.array(V, F64)
    for i, j in ((1, 2), (4, 5), (0, 2), (3, 5), (0, 1), (3, 4), (2, 5), (0, 3), (1, 4), (2, 4), (1, 3), (2, 3)):
        if lam[i] > lam[j]:
            lam[[i, j]] = lam[[j, i]]
            V[:, [i, j]] = V[:, [j, i]]
    for k in range(6):
        big = V[0, k]
        for i in range(1, 6):
            if abs(V[i, k]) > abs(big):
                big = V[i, k]
        if big < 0.0:
            V[:, k] = -V[:, k]
    return lam, V, sweeps


def rodrigues(theta):
    th = np.asarray(theta, F64)
    a2 = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]
    a = math.sqrt(a2)
    R = np.eye(3)
    if a > 0.0:
        Kx = np.array([[0.0, -th[2], th[1]], [th[2], 0.0, -th[0]], [-th[1], th[0], 0.0]])
        R = R + (math.sin(a) / a) * Kx + ((1.0 - math.cos(a)) / a2) * (Kx @ Kx)
    return R


def step(g, c, rho, lam, V, min_ratio, pose):
    """pr_info_step: (pose_out float32[4, 4], delta[6], rank)."""
    g, lam, V = np.asarray(g, F64), np.asarray(lam, F64), np.asarray(V, F64).reshape(6, 6)
    delta, rank = np.zeros(6, F64), 0
    for k in range(6):
        if not (lam[k] > 0.0 and lam[k] > min_ratio * lam[5]):
            continue
        rank += 1
        dot = 0.0
        for i in range(6):
            dot += V[i, k] * g[i]
        delta += V[:, k] * (dot / lam[k])
    pose = np.asarray(pose, F32).reshape(4, 4)
    if rank == 0:
        return pose.copy(), delta, 0
    rho, cc = F64(F32(rho)), np.asarray(c, F32).astype(F64)
    R = rodrigues(delta[:3] / rho)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = 1000.0 * ((cc - R @ cc) + delta[3:])
    out = E @ pose.astype(F64)
    out[3] = pose[3]
    return out.astype(F32), delta, rank


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------------
def refine(surface, contour, poses, iterations, weight, min_ratio, min_used):
    """api.refine_contours' loop: surface(poses) -> list of POSE_INFO records, contour(poses) -> list of (counts dict, POSE_INFO record)."""
    poses = np.asarray(poses, F32).reshape(-1, 4, 4).copy()
    live = np.ones(len(poses), bool)
    hist = dict(rank=[], used=[], rms_px=[], surface_lambda=[], combined_lambda=[])
    for _ in range(iterations):
        surf, con = surface(poses), contour(poses)
        ranks, useds, rms, sl, cl = [], [], [], [], []
        for i in range(len(poses)):
            counts, cinfo = con[i]
            both = combine(surf[i], 1.0, cinfo, weight)
            lam, V, _ = jacobi(both["H"])
            new, _, rank = step(both["g"], both["c"], both["rho"], lam, V, min_ratio, poses[i])
            live[i] &= counts["used"] >= min_used and int(surf[i]["n_valid"]) > 0
            if live[i]:
                poses[i] = new
            ranks.append(rank)
            useds.append(counts["used"])
            rms.append(math.sqrt(counts["sum_d2"] / counts["used"]) if counts["used"] else float("nan"))
            sl.append(jacobi(surf[i]["H"])[0])
            cl.append(lam)
        for key, v in (("rank", ranks), ("used", useds), ("rms_px", rms), ("surface_lambda", sl), ("combined_lambda", cl)):
            hist[key].append(np.array(v))
    return poses, {k: np.array(v) for k, v in hist.items()}


# ---- a plate in front of a wall ------------------------------------------------------------------------------------------------------------------
PLATE = dict(W=160, H=120, K=np.array([200.0, 0.0, 80.0, 0.0, 200.0, 60.0, 0.0, 0.0, 1.0], F32), z_mm=1000.0, wall_mm=1050, half=(100.0, 70.0),
             shift_mm=(24.0, 18.0), angle=0.05, weight=1.0, rho=0.1, radius=8, iterations=8, tau=5, jump=10, min_ratio=1e-6, min_used=8,
             max_dist_diff=0.01)


def plate_tris():
    """Two triangles: a 200 x 140 mm plate in the model's z = 0 plane, centred at the origin; both windings, so it renders from either side."""
    hx, hy = PLATE["half"]
    a, b, c, d = (-hx, -hy, 0.0), (hx, -hy, 0.0), (hx, hy, 0.0), (-hx, hy, 0.0)
    return np.array([[a, b, c], [a, c, d], [a, c, b], [a, d, c]], F32)


def plate_poses():
    """(true pose, start pose): fronto-parallel at z_mm; the start 30 mm (6 px at this depth) off in the plane and 0.05 rad rotated in it."""
    true = np.eye(4, dtype=F64)
    true[2, 3] = PLATE["z_mm"]
    start = true.copy()
    ca, sa = math.cos(PLATE["angle"]), math.sin(PLATE["angle"])
    start[:2, :2] = [[ca, -sa], [sa, ca]]
    start[0, 3], start[1, 3] = PLATE["shift_mm"]
    return true.astype(F32), start.astype(F32)


def plate_scene(render_true):
    """The frame: the plate's render at the true pose, the wall everywhere else.  int32."""
    return np.where(render_true > 0, render_true, PLATE["wall_mm"]).astype(np.int32)


def plate_errors(pose, true):
    """(in-plane translation error in mm, in-plane rotation error in radians) of a pose against the true one."""
    p, t = np.asarray(pose, F64).reshape(4, 4), np.asarray(true, F64).reshape(4, 4)
    R = p[:3, :3] @ t[:3, :3].T
    return float(np.hypot(p[0, 3] - t[0, 3], p[1, 3] - t[1, 3])), abs(math.atan2(R[1, 0], R[0, 0]))


def plane_surface(renders, scene, K, cs, rho, max_dist_diff):
    """The point-to-plane records of renders against a frame of fronto-parallel surfaces (normal (0, 0, -1) everywhere), projective association: the
    cloud point of a rendered pixel against the scene point of the same pixel, accepted within max_dist_diff.  float32 back-projection as the
    cloud extraction does it, then info_ref's terms."""
    k = np.asarray(K, F32).reshape(-1)
    out = []
    for i, img in enumerate(renders):
        ys, xs = np.nonzero(img > 0)

        def back(depth):
            z = depth.astype(F32) / F32(1000.0)
            return np.stack([(xs.astype(F32) - k[2]) / k[0] * z, (ys.astype(F32) - k[5]) / k[4] * z, z], 1)
        cloud, d = back(img[ys, xs]), back(scene[ys, xs])
        n = np.tile(np.array([0.0, 0.0, -1.0], F32), (len(xs), 1))
        diff = (d - cloud).astype(F64)
        valid = (scene[ys, xs] > 0) & ((diff ** 2).sum(1) < max_dist_diff ** 2)
        out.append(info_of(I.record(cloud, (d, n, valid), None, cs[i], rho), cs[i], rho))
    return out
