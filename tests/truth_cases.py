"""Inputs, bounds and assertions shared by test_truth_host.py (the oracle against tests/truth_ref.py) and test_truth_gpu.py (the kernels against
it, directly): the same scenes, the same assertion with the same bound, applied to whoever produced the output.

Every bound below is the ORACLE's own largest deviation from the truth over these inputs, measured on the CPU, plus a quarter of it (the margin is
for the device's identical arithmetic on other inputs, never for the code under test); measured values, bounds and band shares are listed in
profiles/truth/README.md.  Every check prints its figures before it asserts (pytest -s shows them)."""
import functools

import numpy as np

import truth_ref as T
from gpu_common import random_mesh, random_pose

# ---- bounds (profiles/truth/README.md) ------------------------------------------------------------------------------------------------------
RENDER_DEV_MEASURED = 0.499993                      # mm: largest |d - z64| of the oracle's render over the 20 views and their ROIs -- the rounding to a millimetre
RENDER_BOUND = 1.25 * RENDER_DEV_MEASURED            # = 0.5 + m with m = 0.125 mm
CLOUD_REL_MEASURED = 1.472e-7                        # largest |c - c64| / |c64| of a back-projected coordinate (2.5 units of 2^-24: subtraction, division, product, d / 1000)
CLOUD_REL_BOUND = 1.25 * CLOUD_REL_MEASURED
NORMAL_ANGLE_MEASURED_DEG = 2.9045                   # largest angle between get_normal and the true normal, planes and sphere: millimetre quantisation over a 5-pixel arm
NORMAL_ANGLE_BOUND_DEG = 1.25 * NORMAL_ANGLE_MEASURED_DEG
# length of a normal: n * (1 / sqrt(nx^2 + ny^2 + nz^2)) in float32 -- the sum carries at most 2.5 roundings (1.25 u after the root), the root, the
# reciprocal and the product one each: 4.25 u, u = 2^-24.  Reasoned, not measured; 8 u asked.
NORMAL_LEN_TOL = 8 * 2.0 ** -24

EDGE_BAND, EDGE_CAP = 1e-3, 0.01                     # smallest deciding barycentric coordinate; share of a scene's pixels it may leave out
PIXEL_BAND, GATE_BAND, LOOKUP_CAP = 1e-3, 1e-5, 0.02  # px, m; share of a cloud the two may leave out


def say(*a):
    print("[truth]", *a)


# ---- render ---------------------------------------------------------------------------------------------------------------------------------
RENDER_FRAMES = [(1, 97, 61), (2, 64, 48), (3, 130, 77), (6, 65, 65)]                  # seed, W, H: test_render_random_scenes' scenes at 200 triangles
DISTANCES = (300.0, 150.0, 90.0, 600.0, 45.0)


@functools.lru_cache(maxsize=None)
def render_scene(seed, W, H):
    """One random_mesh / random_pose scene: off-centre principal point, fx != fy, five poses.  Per pose ("view"): the triangles with all three
    vertices beyond z = 1 -- the reference does not clip and the ray caster does not model what it draws of a triangle that reaches behind the
    camera, so those stay parity-only (test_render_gpu.py) -- and the truth of the full frame."""
    rng = np.random.default_rng(seed)
    K = np.array([rng.uniform(0.7, 1.6) * W, 0, W / 2 + rng.uniform(-9, 9), 0, rng.uniform(0.7, 1.6) * W, H / 2 + rng.uniform(-9, 9), 0, 0, 1], np.float32)
    tris = random_mesh(rng, 200, 40.0)
    views = []
    for dist in DISTANCES:
        pose = random_pose(rng, dist)
        cam = T.camera_tris(tris, pose)
        keep = T.in_front(cam)
        z, edge = T.raycast(cam[keep], K, W, H)
        views.append(dict(pose=pose, tris=np.ascontiguousarray(tris[keep]), cam=cam[keep], z=z, edge=edge))
    rois = [(0, H // 3, W, 1), (W // 2, H // 2, W - W // 2, H - H // 2)]            # a single row; a window that touches the last row and column
    return dict(K=K, W=W, H=H, views=views, rois=rois)


def window(a, roi):
    x, y, w, h = roi
    return a[y:y + h, x:x + w]


def check_render(img, z, edge, what, cap=True):
    """Outside the edge band: drawn <=> hit, exactly, and |d - z64| <= RENDER_BOUND.  cap: the band leaves out at most EDGE_CAP of the pixels (asked
    of a scene's full frame; a window of one row has 97 pixels)."""
    img = np.asarray(img).astype(np.int64)
    assert img.shape == z.shape, (img.shape, z.shape)
    band = edge < EDGE_BAND
    hit, drawn = np.isfinite(z), img > 0
    wrong = int(((drawn != hit) & ~band).sum())
    both = drawn & hit & ~band
    dev = float(np.abs(img - np.where(hit, z, 0.0))[both].max()) if both.any() else 0.0
    say(f"render {what}: {img.size} px, {int(hit.sum())} hit, band {int(band.sum())} ({band.mean():.4f}), coverage disagreements {wrong}, max |d - z64| {dev:.6f} mm")
    if cap:
        assert band.mean() <= EDGE_CAP, (what, band.mean())
    assert wrong == 0, (what, wrong)
    assert dev <= RENDER_BOUND, (what, dev)
    return dev, float(band.mean())


def fused_size_bounds(z, edge):
    """What the fused path's cloud size may be: hits_outside_band <= size <= hits_outside_band + band_pixels."""
    band = edge < EDGE_BAND
    lo = int((np.isfinite(z) & ~band).sum())
    return lo, lo + int(band.sum())


# ---- back-projection ------------------------------------------------------------------------------------------------------------------------
def cloud_cases():
    """(depth, K, stride, tl_x, tl_y): both depth types, strides 1 / 2 / 3 / 7, three offsets, frames 97 x 61, 33 x 2 and 1 x 1 (a stride beyond the
    frame gives an empty grid); int32 images carry a row of negative depths (not > 0)."""
    out = []
    for W, H in ((97, 61), (33, 2), (1, 1)):
        rng = np.random.default_rng(W * H)
        base = rng.integers(0, 3, size=(H, W)) * rng.integers(200, 3000, size=(H, W))
        base[0, 0] = 731
        K = np.array([80, 0, W / 2 + 1.3, 0, 82, H / 2 - 0.7, 0, 0, 1], np.float32)
        for dt in (np.int32, np.uint16):
            d = base.astype(dt)
            if dt == np.int32 and H > 1:
                d[H // 2, :] = -7
            for stride in (1, 2, 3, 7):
                for tl in ((0, 0), (17, 5), (5, 9)):
                    out.append((d, K, stride, tl[0], tl[1]))
    return out


def check_cloud(got, depth, K, stride, tl_x, tl_y, what):
    """Number of points and their order exact (the truth walks the grid row-major; a point of another cell is off by a pixel's width, not by a
    rounding), every coordinate within CLOUD_REL_BOUND of the float64 value, relatively."""
    want, _ = T.backproject(depth, K, stride, tl_x, tl_y)
    got = np.asarray(got, np.float64).reshape(-1, 3)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if len(want) == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == 0, 0.0, np.inf))
    worst = float(rel.max())
    assert worst <= CLOUD_REL_BOUND, (what, worst)
    return worst


# ---- render, then back-project: the pin of the row convention ------------------------------------------------------------------------------------
def sloped_scene():
    """A square of 80 mm tilted 50 degrees about the camera's x axis, 300 mm away: depth changes by tan(50) * z / fy ~ 4 mm per image row."""
    W, H = 64, 48
    K = np.array([71.0, 0, 30.6, 0, 74.0, 25.3, 0, 0, 1], np.float32)
    q = np.array([[-40, -40, 0], [40, -40, 0], [40, 40, 0], [-40, 40, 0]], np.float32)
    tris = np.ascontiguousarray(np.stack([q[[0, 1, 2]], q[[0, 2, 3]]]))
    a = np.deg2rad(50.0)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], np.float32)
    pose[:3, 3] = [3.0, -2.0, 300.0]
    return dict(K=K, W=W, H=H, tris=tris, pose=pose, cam=T.camera_tris(tris, pose))


def ray_residuals(cloud, cam, K, rows):
    """|z of a cloud point - z of the mesh along the point's ray| in mm, the point first moved by (0, rows * z / fy, 0): (residuals, edge values)."""
    P = np.asarray(cloud, np.float64).reshape(-1, 3)
    fy = float(np.asarray(K).reshape(-1)[4])
    dirs = np.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2] + rows / fy, np.ones(len(P))], 1)
    zt, edge = T.cast(cam, dirs)
    return np.abs(P[:, 2] * 1000.0 - zt), edge


def check_row_pin(cloud, cam, K, frame_pixels, what, sloped=False):
    """Every cloud point moved by (0, +z/fy, 0) -- one image row -- lies on the posed mesh along its ray within the render bound; unmoved it does
    not: on the sloped scene the median residual is above 0.5 mm (what the rounding alone could explain).  The edge band may leave out EDGE_CAP of
    the scene's frame_pixels, as in check_render."""
    res, edge = ray_residuals(cloud, cam, K, T.RENDER_ROW_OFFSET)
    clear = edge >= EDGE_BAND
    worst = float(res[clear].max())
    raw, _ = ray_residuals(cloud, cam, K, 0)
    on = np.isfinite(raw)
    med = float(np.median(raw[on])) if on.any() else np.inf
    say(f"row pin {what}: {len(res)} points, band {int((~clear).sum())}, moved one row: max residual {worst:.5f} mm; unmoved: {int(on.sum())} still meet the mesh, median residual {med:.3f} mm")
    assert len(res) > 100 and (~clear).sum() <= EDGE_CAP * frame_pixels, (what, len(res), int((~clear).sum()))
    assert worst <= RENDER_BOUND, (what, worst)
    if sloped:
        assert on.mean() > 0.8 and med > 0.5, (what, on.mean(), med)
    return worst, med


# ---- normals --------------------------------------------------------------------------------------------------------------------------------
NORMAL_W, NORMAL_H = 64, 48
NORMAL_K = np.array([520.0, 0, 30.7, 0, 505.0, 25.2, 0, 0, 1], np.float32)


@functools.lru_cache(maxsize=None)
def normal_cases():
    """(name, depth in whole mm as int64, true normal per pixel): planes at five tilts 800 mm away and a sphere; a block of every image is pushed
    beyond the 2000 mm gate."""
    out = []
    for n in ((0, 0, -1), (0.3, 0, -1), (0, -0.5, -1), (0.4, 0.7, -1), (-1.1, 0.2, -1)):
        z, nt = T.plane_depth(NORMAL_K, NORMAL_W, NORMAL_H, n, 800.0)
        out.append((f"plane{n}", z, nt))
    z, nt = T.sphere_depth(NORMAL_K, NORMAL_W, NORMAL_H, (6.0, -4.0, 900.0), 150.0)
    out.append(("sphere", z, nt))
    res = []
    for name, z, nt in out:
        d = np.rint(z).astype(np.int64)
        d[30:40, 40:52] = 2500
        res.append((name, d, nt))
    return res


_TAPS = [(-5, -5), (0, -5), (5, -5), (-5, 0), (5, 0), (-5, 5), (0, 5), (5, 5)]              # (dx, dy), radius 5


def tap_gates(d16):
    """For every pixel inside the 5-pixel border rule (rows 5 .. H - 7, columns alike): which of the eight taps pass |d_tap - d| < 50, as a bit set."""
    d = np.asarray(d16).astype(np.int64)
    H, W = d.shape
    inside = np.zeros((H, W), bool)
    inside[5:H - 6, 5:W - 6] = True
    bits = np.zeros((H, W), np.int64)
    c = d[5:H - 6, 5:W - 6]
    for k, (dx, dy) in enumerate(_TAPS):
        t = d[5 + dy:H - 6 + dy, 5 + dx:W - 6 + dx]
        bits[5:H - 6, 5:W - 6] |= (np.abs(t - c) < 50).astype(np.int64) << k
    return inside, bits


def check_normals(normal, depth, n_true, what):
    """Inside the border rule, wherever the pixel is nearer than 2000 mm and all eight taps pass the 50 mm gate: unit length within float rounding,
    turned towards the camera like the true normal (n . n_true > 0, n_true.z < 0), within NORMAL_ANGLE_BOUND_DEG of it.  The border and the pixels at
    2000 mm or beyond: exactly zero."""
    H, W = depth.shape
    n = np.asarray(normal, np.float64).reshape(H, W, 3)
    d16 = np.clip(depth, 0, 65535)
    inside, bits = tap_gates(d16)
    assert not n[~inside].any(), what
    assert not n[inside & (d16 >= 2000)].any(), what
    sel = inside & (d16 < 2000) & (d16 > 0) & (bits == 255)
    assert sel.sum() > 500, (what, sel.sum())
    assert (n_true[sel][:, 2] < 0).all()
    length = np.linalg.norm(n[sel], axis=1)
    dot = (n[sel] * n_true[sel]).sum(1)
    ang = float(np.degrees(np.arccos(np.clip(dot / length, -1, 1))).max())
    say(f"normals {what}: {int(sel.sum())} px, max | |n| - 1 | {np.abs(length - 1).max():.2e}, min n.n_true {dot.min():.4f}, max angle {ang:.4f} deg")
    assert np.abs(length - 1).max() <= NORMAL_LEN_TOL, (what, np.abs(length - 1).max())
    assert (dot > 0).all(), what
    assert ang <= NORMAL_ANGLE_BOUND_DEG, (what, ang)
    return ang


def check_scene_points(pcd, depth, K, what):
    """Scene points of dep2pcd (common.h:47-61), one per pixel: the truth's back-projection where the depth is non-zero, (0, 0, 0) elsewhere."""
    H, W = depth.shape
    want = np.zeros((H, W, 3))
    pts, cells = T.backproject(np.clip(depth, 0, None), K)
    want[cells[:, 1], cells[:, 0]] = pts
    got = np.asarray(pcd, np.float64).reshape(H, W, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == 0, 0.0, np.inf))
    assert rel.max() <= CLOUD_REL_BOUND, (what, rel.max())
    return float(rel.max())


def nn_points_to_pixels(pcd, normal, K, W, H):
    """A kd-tree scene stores its points in tree order: put every point back on its pixel (the nearest pixel centre to its projection, which is a
    whole number up to rounding).  Returns per-pixel (points, normals, mask of the pixels that received a point); no pixel may receive two."""
    fx, fy, cx, cy = (float(v) for v in np.asarray(K).reshape(-1)[[0, 4, 2, 5]])
    P = np.asarray(pcd, np.float64).reshape(-1, 3)
    u = P[:, 0] / P[:, 2] * fx + cx
    v = P[:, 1] / P[:, 2] * fy + cy
    px, py = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    assert np.abs(u - px).max() < 1e-3 and np.abs(v - py).max() < 1e-3
    assert (px >= 0).all() and (px < W).all() and (py >= 0).all() and (py < H).all()
    flat = py * W + px
    assert len(np.unique(flat)) == len(flat)
    pts, nrm, mask = np.zeros((H * W, 3)), np.zeros((H * W, 3)), np.zeros(H * W, bool)
    pts[flat], nrm[flat], mask[flat] = P, np.asarray(normal, np.float64).reshape(-1, 3), True
    return pts.reshape(H, W, 3), nrm.reshape(H, W, 3), mask.reshape(H, W)


# ---- noise: every subset of the eight tap gates -------------------------------------------------------------------------------------------------
NOISE_W, NOISE_H = 130, 77


@functools.lru_cache(maxsize=None)
def noise_depth():
    """Depths drawn evenly from 1000 .. 1170 mm: a tap passes the 50 mm gate with probability one half, independently enough that all 256 subsets
    of the eight gates occur among the 7 854 pixels inside the border (asserted in test_truth_host.py).  No truth applies: device parity's input."""
    return np.random.default_rng(256).integers(1000, 1171, size=(NOISE_H, NOISE_W)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def noise_depth_wide():
    """The same image as int32 with negative values and values above 65535 sprinkled in (the conversion to uint16 saturates)."""
    d = noise_depth().copy()
    rng = np.random.default_rng(257)
    r = rng.random(d.shape)
    d[r < 0.04] = -rng.integers(1, 100000, size=int((r < 0.04).sum()))
    hi = (r >= 0.04) & (r < 0.08)
    d[hi] = 65536 + rng.integers(0, 100000, size=int(hi.sum()))
    return d


def gate_subset_counts(d16):
    inside, bits = tap_gates(d16)
    return np.bincount(bits[inside], minlength=256)


# ---- projective lookup, point by point -------------------------------------------------------------------------------------------------------
LOOKUP_W, LOOKUP_H = 64, 48
LOOKUP_K = np.array([70.0, 0, 31.3, 0, 75.0, 24.6, 0, 0, 1], np.float32)
LOOKUP_MAX_DIST = float(np.float32(0.1))
LOOKUP_WINDOWS = {"whole": (0, 0, LOOKUP_W, LOOKUP_H), "cropped": (7, 5, 41, 29)}
SHALLOW = (30, 20, 16, 12)                                 # x, y, w, h of the region with depths of 1 .. 90 mm (inside both windows)


@functools.lru_cache(maxsize=None)
def lookup_depth():
    yy, xx = np.mgrid[0:LOOKUP_H, 0:LOOKUP_W]
    d = np.rint(600 + 1.5 * xx - 0.8 * yy + 6.0 * np.sin(xx / 5.0) * np.cos(yy / 7.0)).astype(np.int32)
    d[3:9, 50:60] = 0                                      # a hole
    x, y, w, h = SHALLOW
    d[y:y + h, x:x + w] = np.random.default_rng(90).integers(1, 91, size=(h, w))
    return d


def pixel_code(w, h):
    """normal[pixel] = (1, px / 1024, py / 1024): with it, row 3 of a point's terms (J3 * J3..5, sums 15 .. 17 of icp_accumulate.h) reads
    1, px / 1024, py / 1024 exactly, whatever the scene point is."""
    n = np.empty((h, w, 3), np.float32)
    n[..., 0] = 1.0
    n[..., 1] = (np.arange(w, dtype=np.float32) / np.float32(1024))[None, :]
    n[..., 2] = (np.arange(h, dtype=np.float32) / np.float32(1024))[:, None]
    return np.ascontiguousarray(n.reshape(-1, 3))


def decode_terms(rows29):
    """(matched, px, py) from (n, 29) per-point terms under pixel_code; px = py = -1 where nothing matched."""
    r = np.asarray(rows29, np.float64).reshape(-1, 29)
    m = r[:, 28] == 1.0
    assert ((r[:, 28] == 0.0) | m).all()
    assert (r[m, 15] == 1.0).all() and not r[~m].any()
    px, py = r[:, 16] * 1024.0, r[:, 17] * 1024.0
    assert (px == np.rint(px)).all() and (py == np.rint(py)).all()
    return m, np.where(m, px, -1).astype(np.int64), np.where(m, py, -1).astype(np.int64)


def _aim(u, v, z, tl):
    """The float32 point whose projection into the window at tl is (u, v) (common.h:63-73: u = x/z*fx + cx - tl_x + 0.5), at depth z."""
    fx, fy, cx, cy = (float(LOOKUP_K[i]) for i in (0, 4, 2, 5))
    z = np.asarray(z, np.float32).astype(np.float64) * np.ones_like(np.asarray(u, np.float64))
    return np.stack([(u + tl[0] - 0.5 - cx) / fx * z, (v + tl[1] - 0.5 - cy) / fy * z, z], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lookup_cloud(name):
    """The hard cloud of one window: (points float32 (n, 3), block name per point)."""
    x0, y0, w, h = LOOKUP_WINDOWS[name]
    tl = (x0, y0)
    d = lookup_depth()
    fx, fy = float(LOOKUP_K[0]), float(LOOKUP_K[4])
    rng = np.random.default_rng(len(name))
    blocks = []
    # the scene's own points, jittered in 3-D by up to 0.6 pixel sideways and +- 0.15 m in depth
    pts, _ = T.backproject(d, LOOKUP_K)
    pts = pts + np.stack([rng.uniform(-0.6, 0.6, len(pts)) * pts[:, 2] / fx, rng.uniform(-0.6, 0.6, len(pts)) * pts[:, 2] / fy,
                          rng.uniform(-0.15, 0.15, len(pts))], 1)
    blocks.append(("jitter", pts.astype(np.float32)))
    # projections into (-1.5, 0) and (size - 1, size + 0.5) on both axes, at the depth of the nearest window pixel
    n = 60
    for axis in (0, 1):
        for lo, hi in ((-1.5, 0.0), ((w, h)[axis] - 1.0, (w, h)[axis] + 0.5)):
            a = rng.uniform(lo, hi, n)
            b = np.where(rng.random(n) < 0.25, rng.choice([-1.2, -0.3, (h, w)[axis] - 0.4, (h, w)[axis] + 0.3], n), rng.uniform(0, (h, w)[axis], n))
            u, v = (a, b) if axis == 0 else (b, a)
            dz = d[np.clip(np.trunc(v).astype(int), 0, h - 1) + y0, np.clip(np.trunc(u).astype(int), 0, w - 1) + x0]
            blocks.append(("border", _aim(u, v, np.where(dz > 0, dz, 600) / 1000.0, tl)))
    # pixel centres, z within +- 2e-5 of the depth gate on either side of the surface
    n = 64
    u, v = rng.integers(0, w, n) + 0.5 + rng.uniform(-0.3, 0.3, n), rng.integers(0, h, n) + 0.5 + rng.uniform(-0.3, 0.3, n)
    dz = d[np.trunc(v).astype(int) + y0, np.trunc(u).astype(int) + x0] / 1000.0
    off = rng.choice([-1.0, 1.0], n) * (LOOKUP_MAX_DIST + np.tile(np.array([-2e-5, -1.4e-5, -6e-6, 0.0, 6e-6, 1.4e-5, 2e-5, 1.9e-5]), n // 8))
    blocks.append(("gate", _aim(u, v, dz + off, tl)))
    # the shallow region (depths of 1 .. 90 mm): points at z = 0, -0.05, 1e-39 (denormal) and 1e-30 aimed into it -- with max_dist_diff = 0.1 a
    # surface that close to the camera plane is within reach of them
    sx, sy, sw, sh = SHALLOW
    for zv in (0.0, -0.05, 1e-39, 1e-30):
        n = 60
        u = rng.integers(sx, sx + sw, n) - x0 + 0.5 + rng.uniform(-0.4, 0.4, n)
        v = rng.integers(sy, sy + sh, n) - y0 + 0.5 + rng.uniform(-0.4, 0.4, n)
        p = _aim(u, v, zv, tl)
        if zv == 0.0:
            p[::2, :2] = rng.normal(size=(len(p[::2]), 2)).astype(np.float32) * np.float32(0.01)     # x / 0 = +-inf; the rest 0 / 0 = NaN
        blocks.append((f"z={zv:g}", p))
    return np.ascontiguousarray(np.concatenate([b for _, b in blocks])), np.concatenate([[k] * len(b) for k, b in blocks])


def oracle_lookup_rows(name):
    """callable(points) -> (n, 29): the oracle's terms of one-point clouds against the window's scene with the pixel code for normals."""
    import oracle_lib as O
    x0, y0, w, h = LOOKUP_WINDOWS[name]
    scene = O.ProjScene(lookup_depth(), LOOKUP_K, LOOKUP_MAX_DIST)
    if name != "whole":
        scene = scene.crop((x0, y0, w, h))
    scene.normal[:] = pixel_code(w, h)
    return lambda pts: np.stack([O.sum29(p[None], scene) for p in np.asarray(pts, np.float32).reshape(-1, 3)]) if len(pts) else np.zeros((0, 29), np.float32)


def lookup_truth(name):
    x0, y0, w, h = LOOKUP_WINDOWS[name]
    pts, _ = lookup_cloud(name)
    return T.project(pts, LOOKUP_K, x0, y0, w, h, window(lookup_depth(), (x0, y0, w, h)) / 1000.0, LOOKUP_MAX_DIST)


def check_lookup(rows29, name, what, oracle_rows=None):
    """Outside the boundary band the pixel and the accept / reject decision are truth_ref.project's; inside it they are the oracle's on one-point
    clouds (oracle_rows: callable(points) -> (n, 29); None when the oracle itself is what is being checked).  The band leaves out at most
    LOOKUP_CAP of the cloud."""
    pts, block = lookup_cloud(name)
    tr = lookup_truth(name)
    m, px, py = decode_terms(rows29)
    band = (tr.margin_px < PIXEL_BAND) | (tr.margin_z < GATE_BAND)
    clear = ~band
    bad = clear & ((m != tr.accept) | (tr.accept & ((px != tr.px) | (py != tr.py))))
    per = {str(k): (int((block == k).sum()), int((tr.accept & (block == k)).sum()), int((bad & (block == k)).sum())) for k in dict.fromkeys(block)}
    say(f"lookup {what} {name}: {len(pts)} points, band {int(band.sum())} ({band.mean():.4f}); block: (points, truth accepts, disagreements) {per}")
    assert band.mean() <= LOOKUP_CAP, (what, name, band.mean())
    assert tr.accept[clear].sum() > 500
    assert not bad.any(), (what, name, per, pts[bad][:5])
    if oracle_rows is not None and band.any():
        om, opx, opy = decode_terms(oracle_rows(pts[band]))
        assert np.array_equal(m[band], om) and np.array_equal(px[band], opx) and np.array_equal(py[band], opy), (what, name)
    return float(band.mean())
