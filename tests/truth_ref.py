"""Float64 geometry -- TEST INFRASTRUCTURE: a second reference that shares no code with oracle/pose_oracle.c.

The oracle restates the reference in its own float32 arithmetic, and the kernels are held to the oracle bit for bit; a misunderstanding
the two share (a flipped row, a half pixel, a truncation for a rounding, a normal of the wrong sign) is invisible to parity.  What is here
is the geometry itself: rays, planes, spheres and the pinhole projection in plain numpy, float64 throughout, in whatever operand order
numpy likes.  Oracle and kernels are held to it within bounds that are MEASURED on the oracle (profiles/truth/README.md).

Conventions (all from the reference; DESIGN.md section 1 "Image rows"):
  camera frame x right, y down, z forward; K = (fx 0 cx / 0 fy cy / 0 0 1); depths in mm (renders) or m (clouds, scenes);
  back-projection and the projective lookup read pixel (u, v) as the ray ((u - cx)/fx, (v - cy)/fy, 1);
  a RENDER's row v holds the surface along the ray of row v + RENDER_ROW_OFFSET.
"""
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
