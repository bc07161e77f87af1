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


def _aim(u, v, z, tl, K=LOOKUP_K):
    """The float32 point whose projection into the window at tl is (u, v) (common.h:63-73: u = x/z*fx + cx - tl_x + 0.5), at depth z."""
    fx, fy, cx, cy = (float(K[i]) for i in (0, 4, 2, 5))
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


# =================================================================================================================================================
#  The refinement loop: per-point terms, the pending update, the 29 sums, the loop and its fixed point, the fused path
# =================================================================================================================================================
U24 = 2.0 ** -24

# ---- bounds: the oracle's largest deviation over the inputs below (test_truth_host.py re-measures each and asserts it has not grown), times 1.25 ----
TERM_UNITS_MEASURED = 3.944                          # |t32 - t64| of one of a point's 29 terms, in units of 2^-24 of the term's scale (truth_ref.point_to_plane_terms)
MOVED_UNITS_MEASURED = 6.575                         # |p32 - (R p + t)| of a coordinate after the pending update, in units of 2^-24 of sum |m_i x_i| + |t|
MOVED_GIVEN_UNITS_MEASURED = 2.840                    # the same for an update GIVEN as float32 values (no solve in between)
SUM_UNITS_MEASURED = {1024: 2.454, 3072: 2.449}      # |S32 - S64| of a sum in the canonical tree, in units of 2^-24 of the summed scales, per points_per_block
TRAJ_ADD_MEASURED_MM = 1.234e-4                      # mean |T32 p - T64 p| over cloud A after 1, 5 or 20 iterations, mm (a random walk of float32 roundings: one figure for all N)
FIXED_ADD_MEASURED_MM = {1: 0.5316, 5: 1.243e-4, 20: 1.243e-4}   # mean |T32 p - M^-1 p| over cloud A after N iterations, mm: distance from the known motion (the float64 loop: 0.5315, 3.8e-6, 3.8e-6)
# |rmse32 - rmse64| / rmse64 after N iterations on cloud A.  From 5 iterations on the loop sits at its fixed point, where the residual IS the float32 rounding of the
# cloud and of the scene points (rmse 7e-8 m in float32 against 2.6e-8 m in float64): the figure says that, and holds the rmse to the same order of magnitude.
RMSE_REL_MEASURED = {1: 3.110e-6, 5: 1.770, 20: 1.770}
FUSED_ADD_MEASURED_MM = 2.238e-4                     # mean |T32 p - T64 p| over a hypothesis' cloud after 20 iterations, scene B, mm
FUSED_RMSE_REL_MEASURED = 1.430e-5                   # |rmse32 - rmse64| / rmse64 of a hypothesis after 20 iterations, scene B


def bound(measured):
    return 1.25 * measured


# kd-tree association band.  NN_GATE_BAND: the projective gate band (1e-5 m) expressed in d2 at the gate, 2 * max_dist * 1e-5.  NN_GAP_BAND: see
# profiles/truth/README.md "Bands of the loop".
NN_GAP_BAND = 1e-4
NN_GATE_BAND = 2.0 * LOOKUP_MAX_DIST * GATE_BAND
TERM_CAP = 0.02                                      # share of a cloud (its gate blocks included) that the band may leave out of a per-point test

ICP_W, ICP_H = 96, 72
ICP_K = np.array([90.0, 0, 47.3, 0, 90.0, 35.6, 0, 0, 1], np.float32)
ICP_MAX_DIST = LOOKUP_MAX_DIST
ICP_WINDOWS = {"whole": (0, 0, ICP_W, ICP_H), "cropped": (9, 7, 71, 51)}
ICP_PPB = 3072
SUM_PPBS = (1024, 3072)
SUM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073)
LOOP_ITERATIONS = (1, 5, 20)


@functools.lru_cache(maxsize=None)
def scene_a_depth():
    """Scene A: a floor, a wall and a sphere in front of them, the nearest surface per pixel in whole millimetres (470 .. 918)."""
    zs = []
    for n, z0 in (((0.0, -0.6, -1.0), 700.0), ((0.7, 0.1, -1.0), 720.0)):
        z, _ = T.plane_depth(ICP_K, ICP_W, ICP_H, n, z0)
        zs.append(np.where(z > 0, z, np.inf))
    z, _ = T.sphere_depth(ICP_K, ICP_W, ICP_H, (-10.0, 5.0, 560.0), 90.0)
    zs.append(np.where(z > 0, z, np.inf))
    d = np.rint(np.min(zs, 0)).astype(np.int32)
    assert (int(d.min()), int(d.max())) == (470, 918), (d.min(), d.max())
    d.setflags(write=False)
    return d


def _rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def _about(R, centre, shift):
    """The 4 x 4 motion p -> R (p - centre) + centre + shift."""
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + np.asarray(shift)
    return M


@functools.lru_cache(maxsize=None)
def scene_a_oracle(kind, name="whole"):
    """The oracle's scene A: kind "proj" (whole or cropped) or "nn"."""
    import oracle_lib as O
    if kind == "nn":
        return O.NNScene(scene_a_depth(), ICP_K, ICP_MAX_DIST)
    s = O.ProjScene(scene_a_depth(), ICP_K, ICP_MAX_DIST)
    return s if name == "whole" else s.crop(ICP_WINDOWS[name])


@functools.lru_cache(maxsize=None)
def cloud_a():
    """(points float32 (n, 3), block name per point, the 4 x 4 motion that was applied to the scene points to make block "main").
    main: the scene points whose normal is not zero, turned by 1 degree about (1, 2, 0.5) through their centroid and shifted by (3, -2, 4) mm.
    on: scene points themselves, bit for bit.  flat: points 0.2 % further along the ray of a pixel whose normal is zero.  outside: aimed 2.5 pixels
    outside the frame, 250 mm from the camera (more than 0.2 m from every scene point).  behind: 0.15 m in front of or behind a pixel's surface and
    more than 0.12 m from every scene point.  gate_z: on a pixel's ray, within +- 2e-5 m of the depth gate.  gate_nn: at a distance within +- 2e-5 m
    of the gate from the nearest scene point."""
    d = scene_a_depth()
    ps = scene_a_oracle("proj")
    sp = ps.pcd.reshape(ICP_H, ICP_W, 3)
    has_n = ps.normal.any(1).reshape(ICP_H, ICP_W)
    pts, cells = T.backproject(d, ICP_K)
    main64 = pts[has_n[cells[:, 1], cells[:, 0]]]
    assert len(main64) == 5182, len(main64)
    M = _about(_rotation((1.0, 2.0, 0.5), 1.0), main64.mean(0), (0.003, -0.002, 0.004))
    rng = np.random.default_rng(29)
    blocks = [("main", T.rigid_apply(M, main64).astype(np.float32))]
    yy, xx = np.nonzero(has_n)
    k = rng.choice(len(yy), 40, replace=False)
    blocks.append(("on", sp[yy[k], xx[k]].copy()))
    fy_, fx_ = np.nonzero(~has_n & (d > 0))
    inner = (fx_ >= 5) & (fx_ < ICP_W - 6) & (fy_ >= 5) & (fy_ < ICP_H - 6)
    k = np.concatenate([np.nonzero(inner)[0], rng.choice(np.nonzero(~inner)[0], 40, replace=False)])
    blocks.append(("flat", (sp[fy_[k], fx_[k]].astype(np.float64) * 1.002).astype(np.float32)))
    n = 24
    a = rng.choice([-2.0, -2.0, ICP_W + 2.0, ICP_H + 2.0], n)
    side = rng.integers(0, 2, n)
    u = np.where(side == 0, np.where(a < 0, -2.0, ICP_W + 2.0), rng.uniform(0, ICP_W, n))
    v = np.where(side == 1, np.where(a < 0, -2.0, ICP_H + 2.0), rng.uniform(0, ICP_H, n))
    blocks.append(("outside", _aim(u, v, 0.25, (0, 0), ICP_K)))
    n = 120
    px, py = rng.integers(8, ICP_W - 8, n), rng.integers(8, ICP_H - 8, n)
    cand = _aim(px + 0.5, py + 0.5, d[py, px] / 1000.0 + rng.choice([-0.15, 0.15], n), (0, 0), ICP_K)
    far = T.nearest(cand, ps.pcd, ICP_MAX_DIST).d2 > 0.12 ** 2
    assert far.sum() >= 24, far.sum()
    blocks.append(("behind", cand[far][:40]))
    n = 64
    k = rng.choice(len(yy), n, replace=False)
    offs = np.tile(np.array([-2e-5, -1.4e-5, -6e-6, 0.0, 6e-6, 1.4e-5, 2e-5, 1.9e-5]), n // 8)
    blocks.append(("gate_z", _aim(xx[k] + 0.5 + rng.uniform(-0.3, 0.3, n), yy[k] + 0.5 + rng.uniform(-0.3, 0.3, n),
                                  d[yy[k], xx[k]] / 1000.0 + rng.choice([-1.0, 1.0], n) * (ICP_MAX_DIST + offs), (0, 0), ICP_K)))
    # towards the camera from points of the sphere and the floor, then re-aimed from the winner until the distance to the NEAREST scene point is at the gate
    k = rng.choice(len(yy), n, replace=False)
    q = sp[yy[k], xx[k]].astype(np.float64)
    p = q * (1.0 - (ICP_MAX_DIST + offs)[:, None] / np.linalg.norm(q, axis=1, keepdims=True))
    for _ in range(4):
        w = ps.pcd[T.nearest(p, ps.pcd, ICP_MAX_DIST).winner].astype(np.float64)
        dirn = (p - w) / np.linalg.norm(p - w, axis=1, keepdims=True)
        p = w + dirn * (ICP_MAX_DIST + offs)[:, None]
    p = p.astype(np.float32)
    at_gate = np.abs(np.sqrt(T.nearest(p, ps.pcd, ICP_MAX_DIST).d2) - ICP_MAX_DIST) < 3e-5
    assert at_gate.sum() >= 32, at_gate.sum()
    blocks.append(("gate_nn", p[at_gate]))
    cloud = np.ascontiguousarray(np.concatenate([b for _, b in blocks]), np.float32)
    cloud.setflags(write=False)
    return cloud, np.concatenate([[k] * len(b) for k, b in blocks]), M


def cloud_a_main():
    cloud, block, M = cloud_a()
    return cloud[block == "main"], M


def add_mm(Ta, Tb, points):
    """Mean distance in mm between the images of the points (m) under two transforms."""
    return float(np.linalg.norm(T.rigid_apply(Ta, points) - T.rigid_apply(Tb, points), axis=1).mean() * 1000.0)


# ---- association in float64, margins in units of the band --------------------------------------------------------------------------------------
def proj_associate(pcd, window, K=ICP_K, max_dist=ICP_MAX_DIST):
    """truth_ref.project against the window's scene points ((h * w, 3), as whoever is being tested holds them): index = the pixel."""
    x0, y0, w, h = window
    z = np.asarray(pcd, np.float64).reshape(h, w, 3)[..., 2]

    def associate(P):
        tr = T.project(P, K, x0, y0, w, h, z, max_dist)
        return np.where(tr.inside, tr.py * w + tr.px, 0), tr.accept, np.minimum(tr.margin_px / PIXEL_BAND, tr.margin_z / GATE_BAND)
    return associate


def nn_associate(pcd, max_dist=ICP_MAX_DIST):
    """truth_ref.nearest against the scene's points in whatever order the scene stores them."""
    Q = np.asarray(pcd, np.float64).reshape(-1, 3)

    def associate(P):
        nn = T.nearest(P, Q, max_dist)
        return nn.winner, nn.accept, np.minimum(nn.margin_gap / NN_GAP_BAND, nn.margin_gate / NN_GATE_BAND)
    return associate


_truth_terms = {}


def truth_terms(key, cloud, associate, pcd, normal):
    """(terms (n, 29), scales, accept, margin) of a cloud against a scene in float64, zero rows where the truth rejects; cached under `key`."""
    hit = _truth_terms.get(key)
    if hit is None:
        idx, accept, margin = associate(cloud)
        t, sc = T.point_to_plane_terms(cloud, np.asarray(pcd, np.float64).reshape(-1, 3)[idx], np.asarray(normal, np.float64).reshape(-1, 3)[idx])
        t[~accept] = 0.0
        sc[~accept] = 0.0
        for a in (t, sc, accept, margin):
            a.setflags(write=False)
        hit = _truth_terms[key] = (t, sc, accept, margin)
    return hit


def units(got, want, scale):
    """|got - want| in units of 2^-24 of the scale; where the scale is 0 the value must be exact (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / (scale * U24), np.where(err == 0, 0.0, np.inf))


def check_terms(rows29, cloud, block, truth, what, oracle_rows=None, min_accept=500):
    """Per point, outside the association band: the accept / reject decision is the truth's; a rejected point's 29 terms are 0; an accepted
    point's are the float64 terms within bound(TERM_UNITS_MEASURED) units of 2^-24 of their scales (exact where the scale is 0: r and sums
    21 .. 27 of a point that lies on its scene point, sums 0 .. 26 where the scene normal is zero).  Inside the band: the oracle's rows on one-point
    clouds, bit for bit (oracle_rows: callable(points) -> (n, 29); None when the oracle itself is being checked).  The band leaves out at most
    TERM_CAP of the cloud.  Returns (largest deviation in units, band share)."""
    t64, sc, accept, margin = truth
    rows = np.asarray(rows29, np.float32).reshape(-1, 29)
    assert rows.shape == t64.shape, (what, rows.shape, t64.shape)
    band = margin < 1.0
    clear = ~band
    got = rows[:, 28] == 1.0
    assert (got | (rows[:, 28] == 0.0)).all(), what
    wrong = clear & (got != accept)
    un = units(rows, t64, sc)
    worst_col = un[clear].max(0)
    worst = float(worst_col.max())
    per = {str(k): (int((block == k).sum()), int((accept & (block == k)).sum()), int((band & (block == k)).sum()), int((wrong & (block == k)).sum())) for k in dict.fromkeys(block)}
    say(f"terms {what}: {len(rows)} points, left out {int(band.sum())} ({band.mean():.4f}); block: (points, truth accepts, in band, disagreements) {per}")
    say(f"terms {what}: largest |t32 - t64| per column, units of 2^-24 of the scale: {np.array2string(worst_col, precision=2, max_line_width=250)}; max {worst:.3f}")
    assert band.mean() <= TERM_CAP, (what, band.mean())
    assert accept[clear].sum() > min_accept, (what, int(accept[clear].sum()))
    assert not wrong.any(), (what, per, np.asarray(cloud)[wrong][:5])
    assert worst <= bound(TERM_UNITS_MEASURED), (what, worst, int(un[clear].max(1).argmax()))
    # the blocks, by name
    # (in a cropped window an "on" point one pixel outside takes pixel 0 -- truncation -- not its own pixel: only those that lie on their winner count)
    on, flat = clear & (block == "on") & accept & (sc[:, 27] == 0), clear & (block == "flat") & accept
    assert (on.sum() >= 20 or not (block == "on").any()) and not rows[on][:, 21:28].any(), what
    assert not rows[flat][:, :27].any() and (rows[flat][:, 28] == 1.0).all(), what
    assert np.all(units(rows[flat][:, 27], t64[flat][:, 27], sc[flat][:, 27]) <= bound(TERM_UNITS_MEASURED)), what
    for k in ("outside", "behind"):
        sel = clear & (block == k)
        assert not accept[sel].any() and not rows[sel].any(), (what, k)
    if oracle_rows is not None and band.any():
        assert np.array_equal(rows[band].view(np.uint32), np.asarray(oracle_rows(np.asarray(cloud)[band]), np.float32).view(np.uint32)), what
    return worst, float(band.mean())


def oracle_rows_of(scene):
    """callable(points) -> (n, 29): the oracle's terms of one-point clouds (sequential mode, from zero)."""
    import oracle_lib as O
    return lambda pts: np.stack([O.sum29(p[None], scene) for p in np.asarray(pts, np.float32).reshape(-1, 3)]) if len(pts) else np.zeros((0, 29), np.float32)


def given_updates(E_pass0):
    """The two updates the pending-update tests hand over as float32 values: the float64 update of pass 0 of cloud A's main block, and a rotation by
    20 degrees about the camera's axis through the cloud's centroid with a shift of (5, -3, 2) mm."""
    main, _ = cloud_a_main()
    big = _about(_rotation((0.0, 0.0, 1.0), 20.0), main.astype(np.float64).mean(0), (0.005, -0.003, 0.002))
    return {"pass0": np.asarray(E_pass0, np.float32), "20deg": big.astype(np.float32)}


def check_moved(got, M, cloud, what, measured=None):
    """The cloud after the pending update against R p + t in float64 (M as the float32 values the code was given, or the float64 update when the
    code computed its own): every coordinate within bound(measured) units of 2^-24 of sum |m_i x_i| + |t|; measured: MOVED_UNITS_MEASURED (the code solved
    for its own update, whose float32 entries are part of the deviation) unless given."""
    M = np.asarray(M, np.float64).reshape(4, 4)
    P = np.asarray(cloud, np.float64).reshape(-1, 3)
    scale = np.abs(P) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])
    worst = float(units(np.asarray(got).reshape(-1, 3), T.rigid_apply(M, P), scale).max())
    say(f"moved {what}: {len(P)} points, largest deviation {worst:.3f} units of 2^-24 of sum |m x| + |t|")
    assert worst <= bound(MOVED_UNITS_MEASURED if measured is None else measured), (what, worst)
    return worst


def check_sums(row, t64, sc, ppb, what):
    """One row of 29 sums in the canonical tree against the float64 sum of the float64 terms: within bound(SUM_UNITS_MEASURED[ppb]) units of 2^-24
    of the summed scales per column (the count, sum 28, comes out exact under any bound below 1 / n)."""
    un = units(np.asarray(row, np.float32).reshape(29), t64.sum(0), sc.sum(0))
    worst = float(un.max())
    assert worst <= bound(SUM_UNITS_MEASURED[ppb]), (what, ppb, worst, int(un.argmax()))
    return worst


def check_loop(T32, fitness, rmse, truth, N, cloud, known, what):
    """The record of N iterations against the float64 loop: trajectory (ADD between the two composed transforms over the cloud), fitness exactly
    float32(count) / float32(n), rmse relatively, and the distance from the known motion.  Returns (trajectory mm, rmse deviation, fixed point mm)."""
    T32 = np.asarray(T32, np.float64).reshape(4, 4)
    traj = add_mm(T32, truth.Ts[N], cloud)
    fixed = add_mm(T32, known, cloud)
    fixed64 = add_mm(truth.Ts[N], known, cloud)
    want_fit = np.float32(truth.sums[N][28]) / np.float32(len(cloud))
    rel = abs(float(rmse) - truth.rmse[N]) / truth.rmse[N]
    say(f"loop {what} N={N}: trajectory {traj:.3e} mm, fitness {float(fitness):.6f} (truth {float(want_fit):.6f}), rmse {float(rmse):.6e} (truth {truth.rmse[N]:.6e}, rel {rel:.3e}), "
        f"from the known motion {fixed:.3e} mm (float64 loop {fixed64:.3e}); truth: smallest margin {truth.margins[:N + 1].min():.3f} bands, {int(truth.in_band[:N + 1].sum())} band members over {N + 1} passes")
    assert traj <= bound(TRAJ_ADD_MEASURED_MM), (what, N, traj)
    assert np.float32(fitness) == want_fit, (what, N, fitness, want_fit)
    assert rel <= bound(RMSE_REL_MEASURED[N]), (what, N, rel)
    assert fixed <= bound(FIXED_ADD_MEASURED_MM[N]), (what, N, fixed)
    return traj, rel, fixed


# ---- scene B: a small mesh in front of a tilted plane, eight hypotheses -----------------------------------------------------------------------------
FUSED_ITERATIONS = 20
FUSED_MIN_DECIDED = 6


def _octahedron(levels):
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    tris = np.array([[v[a], v[b], v[c]] for a, b, c in f], np.float64)
    for _ in range(levels):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)])
    return tris


@functools.lru_cache(maxsize=None)
def scene_b():
    """mesh (512 triangles, mm): an octahedron subdivided three times, pushed out to a bumpy ellipsoid with half axes of roughly 120, 90 and 70 mm;
    the true pose 520 mm away; the scene depth: truth_ref.raycast of the posed mesh in front of a tilted plane, whole mm; eight hypotheses 0.5 - 3
    degrees (about the object's centre) and 3 mm off the true pose."""
    rng = np.random.default_rng(512)
    t = _octahedron(3)
    u = t / np.linalg.norm(t, axis=2, keepdims=True)
    r = 1.0 + 0.08 * np.sin(3.0 * u[..., 0] + 1.0) * np.cos(4.0 * u[..., 1]) + 0.05 * np.sin(5.0 * u[..., 2])
    tris = np.ascontiguousarray((u * r[..., None] * np.array([120.0, 90.0, 70.0])).astype(np.float32))
    pose = np.eye(4)
    pose[:3, :3] = _rotation((0.3, 1.0, -0.2), 25.0)
    pose[:3, 3] = (4.0, -3.0, 520.0)
    pose = pose.astype(np.float32)
    z, _ = T.raycast(T.camera_tris(tris, pose), ICP_K, ICP_W, ICP_H)
    plane, _ = T.plane_depth(ICP_K, ICP_W, ICP_H, (0.2, -0.1, -1.0), 800.0)
    depth = np.rint(np.minimum(z, plane)).astype(np.int32)
    hyps = []
    for _ in range(8):
        axis, shift = rng.normal(size=3), rng.normal(size=3)
        dT = _about(_rotation(axis, rng.uniform(0.5, 3.0)), pose[:3, 3].astype(np.float64), 3.0 * shift / np.linalg.norm(shift))
        hyps.append((dT @ pose.astype(np.float64)).astype(np.float32))
    depth.setflags(write=False)
    return dict(tris=tris, verts=tris.reshape(-1, 3).astype(np.float64), pose=pose, depth=depth, hyps=np.stack(hyps))


def refined_pose(T_icp, hyp):
    """The hypothesis after the refinement: the ICP transform (m) in front of the pose (mm)."""
    Tm = np.asarray(T_icp, np.float64).reshape(4, 4).copy()
    Tm[:3, 3] *= 1000.0
    return Tm @ np.asarray(hyp, np.float64).reshape(4, 4)


def vertex_add(pose_a, pose_b, verts):
    return float(np.linalg.norm(T.rigid_apply(pose_a, verts) - T.rigid_apply(pose_b, verts), axis=1).mean())


def check_fused(records, clouds, truths, kind, what):
    """records[i] (T, fitness, inlier_rmse) of hypothesis i after FUSED_ITERATIONS against the float64 loop started from clouds[i] (truths[i]).
    A hypothesis is DECIDED when no point was inside the association band in any float64 pass.  kd-tree scene: only decided hypotheses are
    compared, and at least FUSED_MIN_DECIDED must be.  Projective scene: the trajectory, rmse and improvement of EVERY hypothesis are compared and
    only the exact fitness is kept to the decided ones (profiles/truth/README.md "Bands of the loop": a cloud of 950 points nearly always has a
    point within 1e-3 pixel of a pixel's edge in some pass, so the band decides 3 of 8; on these surfaces the neighbouring pixel's point and
    normal move the result by less than the bound, so nothing needs leaving out).
    Returns (compared indices, largest trajectory ADD mm, largest rmse deviation)."""
    sb = scene_b()
    N = FUSED_ITERATIONS
    compared, n_decided, worst, worst_rel = [], 0, 0.0, 0.0
    for i, (rec, cl, tr) in enumerate(zip(records, clouds, truths)):
        decided = int(tr.in_band.sum()) == 0
        n_decided += decided
        T32 = np.asarray(rec["T"], np.float64).reshape(4, 4)
        traj = add_mm(T32, tr.Ts[N], cl)
        want_fit = np.float32(tr.sums[N][28]) / np.float32(len(cl))
        rel = abs(float(rec["inlier_rmse"]) - tr.rmse[N]) / tr.rmse[N]
        start, end = vertex_add(sb["hyps"][i], sb["pose"], sb["verts"]), vertex_add(refined_pose(T32, sb["hyps"][i]), sb["pose"], sb["verts"])
        say(f"fused {what} hypothesis {i}: {len(cl)} points, {'decided' if decided else 'NOT decided'} ({int(tr.in_band.sum())} band members over {N + 1} passes, smallest margin "
            f"{tr.margins.min():.3f} bands), trajectory {traj:.3e} mm, fitness {float(rec['fitness']):.6f} (truth {float(want_fit):.6f}), rmse rel {rel:.3e}, "
            f"ADD to the true pose {start:.2f} -> {end:.2f} mm")
        if not decided and kind != "proj":
            continue
        compared.append(i)
        worst, worst_rel = max(worst, traj), max(worst_rel, rel)
        assert traj <= bound(FUSED_ADD_MEASURED_MM), (what, i, traj)
        if decided:
            assert np.float32(rec["fitness"]) == want_fit, (what, i, rec["fitness"], want_fit)
        assert rel <= bound(FUSED_RMSE_REL_MEASURED), (what, i, rel)
        assert end < start, (what, i, start, end)
    say(f"fused {what}: {n_decided} of {len(records)} decided, compared {compared}, largest trajectory ADD {worst:.3e} mm, largest rmse deviation {worst_rel:.3e}")
    assert len(compared) >= FUSED_MIN_DECIDED, (what, compared)
    return compared, worst, worst_rel


def check_fused_sums(rows0, clouds, assoc, pcd, normal, key, what):
    """Row 0 of every hypothesis (the sums of its first pass, canonical tree at ICP_PPB) against the float64 sums of its cloud."""
    worst = 0.0
    for i, cl in enumerate(clouds):
        t64, sc, _, _ = truth_terms((key, i), cl, assoc, pcd, normal)
        worst = max(worst, check_sums(rows0[i], t64, sc, ICP_PPB, f"{what} hypothesis {i}"))
    say(f"fused sums {what}: first pass of {len(clouds)} hypotheses, largest deviation {worst:.3f} units of 2^-24 of the summed scales")
    return worst
