"""Frames for the support-plane tests (tests/test_planes_host.py, tests/test_planes_gpu.py): analytic planes rendered to a 1 mm depth image in
float64, and small synthetic scenes of random points and normals with planted planes (like _synthetic_scene of tests/test_ppf_gpu.py)."""
import math

import numpy as np

F = np.float32
W, H = 64, 48
K64 = np.array([60.0, 0.0, 31.5, 0.0, 60.0, 23.5, 0.0, 0.0, 1.0], F)      # a wide lens: a 64 x 48 frame sees 0.6 m of a plane at 0.6 m


def rays(w, h, K):
    """float64 [h, w, 3]: the ray (x/z, y/z, 1) of every pixel, as the scene preparation back-projects it"""
    K = np.asarray(K, np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([(u - K[2]) / K[0], (v - K[5]) / K[4], np.ones_like(u)], axis=2)


def plane_depth(w, h, K, n, d):
    """float64 [h, w]: the z (mm) at which every pixel's ray meets the plane n . p = d (n unit, d in mm); inf where it does not in front"""
    den = rays(w, h, K) @ np.asarray(n, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(den != 0, d / den, np.inf)
    return np.where(z > 0, z, np.inf)


def tilted(deg_x, deg_y=0.0):
    """unit normal of the plane z = const turned about the camera's x (then y) axis, pointing at the camera (n . p < 0)"""
    ax, ay = np.deg2rad(deg_x), np.deg2rad(deg_y)
    n = np.array([0.0, 0.0, -1.0])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return Ry @ Rx @ n


def fit_bound(points_mm, n, d, K, w, h):
    """(delta, tan_theta, offset_bound) for a total-least-squares plane through ``points_mm`` (float64 [m, 3]), all samples of the plane n . p = d.

    The depth is rounded to 1 mm, so a sample sits on its pixel's ray r = (x/z, y/z, 1) at most 0.5 mm of z from the plane: at most
    0.5 max|n . r| mm off it.  The moments round every coordinate to 1/16 mm: at most (|nx| + |ny| + |nz|) / 32 mm more; 1e-3 mm covers the
    float32 back-projection (ulp of 1 m in mm: 6e-5, a handful of operations).  delta is the sum.  With a_i the samples' signed distances to
    the true plane (|a_i| <= delta) and b_i their coordinates along any in-plane direction t, both about their means, the fitted plane -- which
    passes through the centroid and minimises the sum of squares -- tilted by theta towards t has residuals cos(theta) a_i - sin(theta) b_i and
    does no worse than the true plane's direction:  sum (cos a_i - sin b_i)^2 <= sum a_i^2, which gives
    tan(theta) (B - A) <= 2 sum a_i b_i <= 2 sqrt(A B), A = sum a_i^2 <= m delta^2, B = sum b_i^2 >= m sigma^2 with sigma^2 the smaller
    eigenvalue of the samples' in-plane covariance.  Hence tan(theta) <= 2 delta sigma / (sigma^2 - delta^2); 1e-6 covers the float32 rounding
    of the normal.  The offset is n_fit . centroid: |offset - d| <= |mean a_i| + |n_fit - n| |centroid| <= delta + tan(theta) |centroid|,
    and 1e-3 mm covers its float32 rounding."""
    n = np.asarray(n, np.float64)
    delta = 0.5 * np.abs(rays(w, h, K) @ n).max() + np.abs(n).sum() / 32.0 + 1e-3
    e1 = np.cross(n, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    b = np.stack([points_mm @ e1, points_mm @ e2], axis=1)
    sigma = math.sqrt(np.linalg.eigvalsh(np.cov(b.T, bias=True))[0])
    assert sigma > 10.0 * delta
    tan_theta = 2.0 * delta * sigma / (sigma * sigma - delta * delta) + 1e-6
    return delta, tan_theta, delta + tan_theta * np.linalg.norm(points_mm.mean(0)) + 1e-3


def one_plane():
    n = tilted(25.0, 10.0)
    z = plane_depth(W, H, K64, n, -600.0)
    return dict(depth=np.rint(z).astype(np.uint16), truth=[(n, -600.0)], owner=np.ones((H, W), np.int64), K=K64)


def two_planes():
    """a floor and a wall meeting in an edge: each pixel sees the nearer one"""
    a, b = (tilted(40.0), -500.0), (tilted(-35.0, 5.0), -560.0)
    za, zb = plane_depth(W, H, K64, *a), plane_depth(W, H, K64, *b)
    z = np.minimum(za, zb)
    return dict(depth=np.rint(z).astype(np.uint16), truth=[a, b], owner=np.where(za <= zb, 1, 2), K=K64)


def plane_with_box():
    """a tilted table with a box on it: the box's top is parallel to the table, 60 mm nearer the camera"""
    n = tilted(20.0)
    z = plane_depth(W, H, K64, n, -650.0)
    top = plane_depth(W, H, K64, n, -590.0)
    owner = np.ones((H, W), np.int64)
    owner[16:34, 22:44] = 0                                         # the box
    z = np.where(owner == 0, top, z)
    return dict(depth=np.rint(z).astype(np.uint16), truth=[(n, -650.0)], owner=owner, K=K64)


def synthetic(w=W, h=H, seed=5, two=True, holes=0.2, bare=0.1):
    """(pcd float32[h, w, 3] metres, normals float32[h, w, 3], depth uint16[h, w], facts): random points and normals with holes, depth without a
    normal, a z <= 0 and a z beyond 65 535 mm, and planted planes.  Plane A (rows 12 .. 27) is z = 0.5 m exactly with the normal (0, 0, -1)
    exactly: every one of its points supports every other with r == 0, so its candidates tie.  Planted on it:
    two identical samples at z = 0.502f (|r| == facts['tau_edge'] exactly; the lower index wins) next to one a float above them, a normal whose dot with (0, 0, -1) is exactly
    0.8f (facts['cos_edge']) next to one a float below.  Plane B (rows 32 .. 45, when ``two``) is tilted, with
    jittered normals."""
    rng = np.random.default_rng(seed)
    pcd = rng.uniform(-0.3, 0.3, (h, w, 3)).astype(F)
    pcd[..., 2] = rng.uniform(0.2, 0.9, (h, w)).astype(F)
    nrm = rng.normal(size=(h, w, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    ra, rb = slice(12, 28), slice(32, 46)
    pcd[ra, :, 2] = F(0.5)
    nrm[ra] = [0, 0, -1]
    if two:
        nb = np.array([0.3, -0.2, -0.9]) / np.linalg.norm([0.3, -0.2, -0.9])
        xy = pcd[rb, :, :2].astype(np.float64)
        pcd[rb, :, 2] = ((-0.7 - xy @ nb[:2]) / nb[2]).astype(F)      # n . p = -0.7 m
        jit = nb + rng.normal(scale=0.02, size=pcd[rb].shape)
        nrm[rb] = (jit / np.linalg.norm(jit, axis=2, keepdims=True)).astype(F)
    hole = rng.random((h, w)) < holes
    pcd[hole] = 0                                                   # holes: no depth (and, as the scene preparation leaves them, no normal)
    nrm[hole] = 0
    nrm[rng.random((h, w)) < bare] = 0                               # depth without a normal
    r0 = ra.start
    pcd[r0, 0] = [0.1, 0.1, 0.5]; nrm[r0, 0] = [0, 0, -1]           # (row r0 and the columns x % 12 == 0 are on the grid of every stride used)
    pcd[r0, 12] = [0.0, 0.05, F(0.502)]; nrm[r0, 12] = [0, 0, -1]   # |r| == tau_edge exactly against plane A; as a candidate it reaches plane A and what lies
    pcd[r0, 24] = pcd[r0, 12]; nrm[r0, 24] = nrm[r0, 12]            # up to 2 tau_edge behind it: the most support -- and its twin, an identical candidate
    pcd[r0, 36] = [0.0, 0.06, np.nextafter(F(0.502), F(1))]; nrm[r0, 36] = [0, 0, -1]
    pcd[r0, 48] = [0.02, 0.0, 0.5]; nrm[r0, 48] = [F(0.6), 0, -F(0.8)]                      # dot == cos_edge exactly
    pcd[r0, 60] = [0.03, 0.0, 0.5]; nrm[r0, 60] = [F(0.6), 0, np.nextafter(-F(0.8), F(0))]
    pcd[1, 2, 2] = -0.4                                             # a depth that is not > 0
    pcd[2, 4] = [0.0, 0.0, 70.0]; nrm[2, 4] = [0, 0, -1]            # beyond 65 535 mm: measured, no sample
    pcd[0, 0] = [0.1, 0.1, 0.45]; nrm[0, 0] = [0, 1e-30, 0]         # one non-zero component is a normal
    tau_edge = F(F(F(0.502) * F(1000.0)) - F(F(0.5) * F(1000.0)))
    depth = np.clip(np.rint(pcd[..., 2].astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
    return pcd, nrm, depth, dict(tau_edge=float(tau_edge), cos_edge=float(F(0.8)), row_a=r0)


def assert_same(got, ref, n_planes):
    """(planes, labels, depth, moments, supports) of the library against the reference's dict, byte for byte"""
    planes, labels, depth, moments, supports = got
    assert len(planes) == len(ref["planes"])
    for g, r in zip(planes, ref["planes"]):
        assert g["normal"].tobytes() == r["normal"].tobytes() and g["offset_mm"].tobytes() == r["offset_mm"].tobytes() and g["rms_mm"].tobytes() == r["rms_mm"].tobytes()
        assert (int(g["candidate"]), int(g["support"]), int(g["labelled"]), int(g["behind"])) == (r["candidate"], r["support"], r["labelled"], r["behind"])
        assert not g["reserved"].any()
    assert moments.tobytes() == ref["moments"].tobytes()
    assert supports.shape == (n_planes, 4096) and supports.tobytes() == ref["supports"].tobytes()
    assert labels.dtype == np.uint8 and labels.tobytes() == ref["labels"].tobytes()
    assert depth.dtype == ref["depth"].dtype and depth.tobytes() == ref["depth"].tobytes()


def synthetic_variants():
    """(id, frame arguments, parameters): between them the strides, the exact edges, the normal test off, the short peel, drop_behind both ways"""
    _, _, _, facts = synthetic()
    edge = dict(tau_mm=facts["tau_edge"], label_tau_mm=facts["tau_edge"], cos_min=facts["cos_edge"], min_support=40)
    return [("stride1_edges", {}, dict(stride=1, cand_stride=1, n_planes=3, drop_behind=False, **edge)),
            ("stride3", {}, dict(stride=3, cand_stride=2, n_planes=2, drop_behind=True, **edge)),
            ("stride4_one_candidate", {}, dict(stride=4, cand_stride=4096, n_planes=1, drop_behind=True, **dict(edge, min_support=3))),
            ("no_normal_test", {}, dict(stride=1, cand_stride=7, n_planes=2, drop_behind=True, **dict(edge, cos_min=-2.0))),
            ("one_plane_three_asked", dict(two=False, seed=9), dict(stride=2, cand_stride=3, n_planes=3, drop_behind=False, **edge))]
