"""Float64 geometry -- TEST INFRASTRUCTURE: a second reference that shares no code with oracle/pose_oracle.c.

The oracle restates the reference in its own float32 arithmetic, and the kernels are held to the oracle bit for bit; a misunderstanding
the two share (a flipped row, a half pixel, a truncation for a rounding, a normal of the wrong sign) is invisible to parity.  What is here
is the geometry itself: rays, planes, spheres, the pinhole projection, and point-to-plane refinement (terms, nearest neighbour, update, loop) in plain numpy, float64 throughout, in whatever operand order
numpy likes.  Oracle and kernels are held to it within bounds that are MEASURED on the oracle (profiles/truth/README.md).

Conventions (all from the reference; DESIGN.md section 1 "Image rows"):
  camera frame x right, y down, z forward; K = (fx 0 cx / 0 fy cy / 0 0 1); depths in mm (renders) or m (clouds, scenes);
  back-projection and the projective lookup read pixel (u, v) as the ray ((u - cx)/fx, (v - cy)/fy, 1);
  a RENDER's row v holds the surface along the ray of row v + RENDER_ROW_OFFSET.
"""
import math
from collections import namedtuple

import numpy as np

# The raster row is py = H - cy - fy*y/z (compute_proj's flipped y, then the viewport's + H/2), and the fragment is written to image row
# H - 1 - py = fy*y/z + cy - 1 (renderer.cpp:170-171, renderer.cu:142: y_to_write = height - 1 - P[1] - roi.y).  The "- 1" makes image row v show
# what back-projection would call row v + 1.  It is the reference's behaviour and stays; the truth models it with this one constant.
RENDER_ROW_OFFSET = 1

INT_MAX = 2 ** 31 - 1


def _k(K):
    K = np.asarray(K, np.float64).reshape(-1)
    return K[0], K[4], K[2], K[5]


def camera_tris(tris, pose):
    """(n, 3, 3) model triangles under a 4x4 pose, in float64 (the float32 inputs are exact in it)."""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    return np.asarray(tris, np.float64).reshape(-1, 3, 3) @ T[:3, :3].T + T[:3, 3]


def in_front(tris_cam, z_min=1.0):
    """Mask of the triangles whose three vertices lie beyond z_min: the reference does not clip, and what it draws of a triangle that
    reaches behind the camera (a wrap-around of the perspective division) is no geometry a ray caster models."""
    return (np.asarray(tris_cam)[:, :, 2] > z_min).all(1)


def raycast(tris_cam, K, W, H, roi=None):
    """Moeller-Trumbore for every pixel of the frame (or of roi = (x, y, w, h)) along ((u - cx)/fx, (v + RENDER_ROW_OFFSET - cy)/fy, 1).

    Returns (z, edge): z[v, u] = the nearest positive z over the triangles the ray hits, in the triangles' unit (inf: no hit);
    edge[v, u] = the smallest |barycentric coordinate that decides inside / outside| over all triangles, i.e. min over triangles of
    |min(b0, b1, b2)| -- a pixel whose edge value is below a band lies that close (in barycentric units) to some triangle's outline, and
    float32 rasterisation may put it on the other side.  Triangles without area are skipped (they have no inside)."""
    fx, fy, cx, cy = _k(K)
    x0, y0, w, h = (0, 0, W, H) if roi is None or roi[2] <= 0 or roi[3] <= 0 else (int(v) for v in roi)
    u = np.arange(x0, x0 + w, dtype=np.float64)
    v = np.arange(y0, y0 + h, dtype=np.float64)
    d = np.empty((h, w, 3))
    d[..., 0] = ((u - cx) / fx)[None, :]
    d[..., 1] = ((v + RENDER_ROW_OFFSET - cy) / fy)[:, None]
    d[..., 2] = 1.0
    z, edge = cast(tris_cam, d.reshape(-1, 3))
    return z.reshape(h, w), edge.reshape(h, w)


def cast(tris_cam, dirs):
    """raycast's two results for rays from the camera along the given (n, 3) directions with z component 1."""
    D = np.asarray(dirs, np.float64).reshape(-1, 3)
    tri = np.asarray(tris_cam, np.float64).reshape(-1, 3, 3)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    tri = tri[np.any(np.cross(e1, e2) != 0, 1)]
    if len(tri) == 0:
        return np.full(len(D), np.inf), np.full(len(D), np.inf)
    # with the ray's origin at the camera, t0 = -v0, and every Moeller-Trumbore term is the ray direction dotted with a vector of the
    # triangle: det = (d x e2).e1 = d.(e2 x e1), b1 = (d x e2).t0 / det = d.(e2 x t0) / det, b2 = d.(t0 x e1) / det, t = e2.(t0 x e1) / det
    e1, e2, t0 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], -tri[:, 0]
    q = np.cross(t0, e1)
    det = D @ np.cross(e2, e1).T                                # (rays, triangles)
    with np.errstate(divide="ignore", invalid="ignore"):
        b1 = (D @ np.cross(e2, t0).T) / det
        b2 = (D @ q.T) / det
        t = (e2 * q).sum(1)[None, :] / det                      # the ray's parameter = z, since the ray's z component is 1
    lo = np.minimum(np.minimum(1.0 - b1 - b2, b1), b2)
    ok = det != 0
    edge = np.where(ok, np.abs(lo), np.inf).min(1)
    z = np.where(ok & (lo >= 0) & (t > 0), t, np.inf).min(1)
    return z, edge


def backproject(depth, K, stride=1, tl_x=0, tl_y=0, empty_int_max=False):
    """The points of icp.cu:249-253: grid cell (x, y) of the W//stride x H//stride grid samples depth[y*stride, x*stride] and becomes
    ((x + tl_x - cx)/fx * z, (y + tl_y - cy)/fy * z, z), z = d/1000 -- the CELL index enters the ray, not the sampled pixel's (the
    reference's rule) -- row-major over the grid, valid cells only (d > 0; with empty_int_max also d != INT_MAX, the raster's "nothing
    drawn" before render's final pass turns it into 0).  Returns (points (n, 3) float64, grid cells (n, 2) as (x, y))."""
    fx, fy, cx, cy = _k(K)
    d = np.asarray(depth)
    H, W = d.shape
    gw, gh = W // stride, H // stride
    s = d[:gh * stride:stride, :gw * stride:stride].astype(np.int64)[:gh, :gw]
    valid = s > 0
    if empty_int_max:
        valid &= s != INT_MAX
    gy, gx = np.nonzero(valid)                                  # row-major
    z = s[gy, gx] / 1000.0
    pts = np.stack([(gx + tl_x - cx) / fx * z, (gy + tl_y - cy) / fy * z, z], 1)
    return pts, np.stack([gx, gy], 1)


def _pixel_rays(K, W, H):
    fx, fy, cx, cy = _k(K)
    r = np.empty((H, W, 3))
    r[..., 0] = ((np.arange(W) - cx) / fx)[None, :]
    r[..., 1] = ((np.arange(H) - cy) / fy)[:, None]
    r[..., 2] = 1.0
    return r


def plane_depth(K, W, H, normal, z0):
    """The plane through (0, 0, z0) mm with the given normal, seen through pixel rays ((u - cx)/fx, (v - cy)/fy, 1).
    Returns (depth in mm, float64, unrounded; unit normal per pixel turned towards the camera: nz < 0)."""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    if n[2] > 0:
        n = -n
    r = _pixel_rays(K, W, H)
    z = (n[2] * z0) / (r @ n)
    return z, np.broadcast_to(n, (H, W, 3)).copy()


def sphere_depth(K, W, H, center, radius):
    """The near surface of a sphere (mm).  Returns (depth in mm, 0 where the ray misses; outward unit normal at the hit, 0 where it misses)."""
    c = np.asarray(center, np.float64)
    r = _pixel_rays(K, W, H)
    a = (r * r).sum(-1)
    b = r @ c
    disc = b * b - a * (c @ c - radius * radius)
    hit = disc > 0
    t = np.where(hit, (b - np.sqrt(np.where(hit, disc, 0.0))) / a, 0.0)
    hit &= t > 0
    z = np.where(hit, t, 0.0)
    n = (r * t[..., None] - c) / radius
    return z, np.where(hit[..., None], n, 0.0)


Projection = namedtuple("Projection", "px py inside margin_px accept margin_z")


def _axis(u, size):
    """One image axis of pcd2dep (common.h:63-73): the pixel int(u) -- truncation, so (-1, 1) is pixel 0 -- and 0 <= p < size; and how far u
    is from the nearest value at which that answer changes: -1, 1, 2, ..., size (the frame limits among them)."""
    fin = np.isfinite(u)
    uu = np.where(fin, u, -2.0)                                 # (any value outside; the margin of a non-finite u is inf below)
    inside = fin & (uu > -1.0) & (uu < size)
    p = np.where(inside, np.trunc(np.where(inside, uu, 0.0)), -1).astype(np.int64)
    f = uu - np.floor(uu)
    m = np.minimum(f, 1.0 - f)                                  # an integer value of u
    m = np.where(np.abs(uu) < 1.0, np.minimum(uu + 1.0, 1.0 - uu), m)          # ... except 0: both sides of it are pixel 0
    m = np.where(uu <= -1.0, -1.0 - uu, m)
    m = np.where(uu >= size, uu - size, m)
    return p, inside, np.where(fin, m, np.inf)


def project(points, K, tl_x, tl_y, W, H, scene_z=None, max_dist_diff=0.1):
    """Scene_projective::query's decisions (depth_scene.h:29-48) for (n, 3) points against a W x H scene window whose top left pixel is
    (tl_x, tl_y): u = x/z*fx + cx - tl_x + 0.5, v alike; the pixel is (int(u), int(v)) if both lie in the window.  With scene_z (the window's
    depths in m, (H, W)) the point is accepted iff the pixel holds a surface (z > 0) no further than max_dist_diff from the point in z.
    margin_px: distance of (u, v) to the nearest value where the pixel or the inside decision changes; margin_z: distance of |sz - dz| from
    max_dist_diff (inf where the gate is never reached).  A point with z = 0 or a non-finite projection is outside, with margin inf."""
    fx, fy, cx, cy = _k(K)
    P = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = P[:, 0] / P[:, 2] * fx + cx - tl_x + 0.5
        v = P[:, 1] / P[:, 2] * fy + cy - tl_y + 0.5
    px, in_x, mx = _axis(u, W)
    py, in_y, my = _axis(v, H)
    inside = in_x & in_y
    margin_px = np.minimum(mx, my)
    accept = np.zeros(len(P), bool)
    margin_z = np.full(len(P), np.inf)
    if scene_z is not None:
        sz = np.asarray(scene_z, np.float64).reshape(H, W)
        dz = sz[np.where(inside, py, 0), np.where(inside, px, 0)]
        gate = np.abs(P[:, 2] - dz)
        surf = inside & (dz > 0)
        accept = surf & (gate <= max_dist_diff)
        margin_z = np.where(surf, np.abs(gate - max_dist_diff), np.inf)
    return Projection(np.where(inside, px, -1), np.where(inside, py, -1), inside, margin_px, accept, margin_z)


# ---- the refinement loop: point-to-plane terms, nearest neighbour, the rigid update -------------------------------------------------------------
def rigid_apply(M, points):
    """R p + t for the 4 x 4 (or 16 values, row-major) M and (n, 3) points."""
    M = np.asarray(M, np.float64).reshape(4, 4)
    return np.asarray(points, np.float64).reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]


_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]          # the 21 slots of the upper triangle, row-major (icp.h:138-206)


def point_to_plane_terms(src, dst, nrm):
    """What one correspondence (source point s, scene point d, scene normal n) adds to the normal equations of point-to-plane ICP, linearised
    about the identity: the residual r = (d - s) . n and its gradient J = (s x n, n) with respect to (rotation vector, translation).
    Returns (terms (n, 29), scales (n, 29)).  Slots, the reference's (icp.h:138-206): 0 .. 20 the upper triangle of J J^T row-major,
    21 .. 26 J r, 27 the squared distance |d - s|^2, 28 the count 1.  A scale is the sum of the magnitudes of what is added and subtracted
    to form the term: |a_i b_i| summed for a dot or cross product component, the product of the factors' scales for a product; float32
    arithmetic in any order misses the term by a few units of 2^-24 of its scale, and where the scale is 0 the term is exactly 0."""
    s = np.asarray(src, np.float64).reshape(-1, 3)
    d = np.asarray(dst, np.float64).reshape(-1, 3)
    n = np.asarray(nrm, np.float64).reshape(-1, 3)
    e = d - s
    r = np.einsum("ij,ij->i", e, n)
    r_scale = np.abs(e * n).sum(1)
    J = np.concatenate([np.cross(s, n), n], 1)
    roll1, roll2 = np.roll(np.abs(s), -1, 1) * np.roll(np.abs(n), -2, 1), np.roll(np.abs(s), -2, 1) * np.roll(np.abs(n), -1, 1)
    J_scale = np.concatenate([roll1 + roll2, np.abs(n)], 1)      # component i of s x n is s[i+1] n[i+2] - s[i+2] n[i+1]
    terms, scales = np.empty((len(s), 29)), np.empty((len(s), 29))
    for k, (a, b) in enumerate(_UPPER):
        terms[:, k], scales[:, k] = J[:, a] * J[:, b], J_scale[:, a] * J_scale[:, b]
    terms[:, 21:27], scales[:, 21:27] = J * r[:, None], J_scale * r_scale[:, None]
    terms[:, 27] = scales[:, 27] = (e * e).sum(1)
    terms[:, 28] = scales[:, 28] = 1.0
    return terms, scales


Nearest = namedtuple("Nearest", "winner d2 accept margin_gap margin_gate")


def nearest(points, scene_points, max_dist, chunk=256):
    """Brute force, in chunks of `chunk` queries: for every point the scene point at the smallest squared distance d2 (pcd_scene.h:60-136
    finds the same one through its tree), accept = d2 < max_dist^2.  margin_gap: (d2 of the runner-up - d2) / d2 of the runner-up, the
    relative gap that another rounding of the two distances would have to bridge to change the winner (1 for a scene of one point or a
    point that lies on its winner); margin_gate: |d2 - max_dist^2|."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    Q = np.asarray(scene_points, np.float64).reshape(-1, 3)
    win, d2, second = np.zeros(len(P), np.int64), np.zeros(len(P)), np.full(len(P), np.inf)
    for a in range(0, len(P), chunk):
        D = (P[a:a + chunk, 0, None] - Q[None, :, 0]) ** 2 + (P[a:a + chunk, 1, None] - Q[None, :, 1]) ** 2 + (P[a:a + chunk, 2, None] - Q[None, :, 2]) ** 2
        w = D.argmin(1)
        rows = np.arange(len(w))
        win[a:a + chunk], d2[a:a + chunk] = w, D[rows, w]
        if len(Q) > 1:
            D[rows, w] = np.inf
            second[a:a + chunk] = D.min(1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second) & (second > 0), (second - d2) / np.where(second > 0, second, 1.0), np.where(np.isfinite(second), 0.0, 1.0))
    g2 = float(max_dist) ** 2
    return Nearest(win, d2, d2 < g2, gap, np.abs(d2 - g2))


def float64_truth(s):
    """The update of 29 sums: np.linalg.solve(A + 0.01 I, b) in float64, A the symmetric matrix whose upper triangle is s[0:21] row-major and
    b = s[21:27]; then Rz Ry Rx from math.sin / math.cos and the translation x[3:6] (icp.cpp:7-27 in exact arithmetic).
    Returns (4 x 4 transform, condition number of A + 0.01 I, x)."""
    s = np.asarray(s, np.float64).reshape(-1)
    A = np.zeros((6, 6))
    for k, (a, b) in enumerate(_UPPER):
        A[a, b] = A[b, a] = s[k]
    A += 0.01 * np.eye(6)
    x = np.linalg.solve(A, s[21:27])
    cx, sx, cy, sy, cz, sz = (math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2]))
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:]
    return T, float(np.linalg.cond(A)), x


Icp = namedtuple("Icp", "T Ts sums margins in_band fitness rmse")


def icp(cloud, associate, scene_points, scene_normals, iterations):
    """Gauss-Newton point-to-plane refinement in float64 (icp.cpp:125-188 with criteria (0, 0, iterations): `iterations` updates, then one more
    pass that only scores).  associate(points) -> (index into the scene arrays, accept, margin) per point, the margin in units of the
    caller's band (below 1: a float32 evaluation may decide otherwise).
    Returns T: the composed transform; Ts[k]: the composed transform after k updates (Ts[0] = identity); sums[k]: the 29 sums of pass k;
    margins[k] / in_band[k]: the smallest margin of pass k and how many points were below 1; fitness[k] = count / n and
    rmse[k] = sqrt(sum 27 / count) of pass k -- the record of a run of k iterations is (Ts[k], fitness[k], rmse[k])."""
    P = np.asarray(cloud, np.float64).reshape(-1, 3).copy()
    Q = np.asarray(scene_points, np.float64).reshape(-1, 3)
    N = np.asarray(scene_normals, np.float64).reshape(-1, 3)
    T = np.eye(4)
    Ts, sums, margins, in_band, fitness, rmse = [T], [], [], [], [], []
    for it in range(iterations + 1):
        idx, accept, margin = associate(P)
        terms, _ = point_to_plane_terms(P[accept], Q[idx[accept]], N[idx[accept]])
        s = terms.sum(0)
        sums.append(s)
        margins.append(float(np.min(margin)) if len(P) else np.inf)
        in_band.append(int((np.asarray(margin) < 1.0).sum()))
        fitness.append(s[28] / max(len(P), 1))
        rmse.append(float(np.sqrt(s[27] / s[28])) if s[28] > 0 else 0.0)
        if it == iterations or s[28] == 0:
            break
        E, _, _ = float64_truth(s)
        P = rigid_apply(E, P)
        T = E @ T
        Ts.append(T)
    return Icp(T, Ts, np.array(sums), np.array(margins), np.array(in_band), np.array(fitness), np.array(rmse))
