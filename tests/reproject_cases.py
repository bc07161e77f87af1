"""The small cases of the reprojection tests (test_reproject_host.py, test_reproject_gpu.py): the smallest shapes at which the scatter's slots of
16 bytes, its heads and tails, the clipped squares, the gates, the z-buffer's tie rule and the resolve's tiles (64 x 16) and windows can still go
wrong.  A case is (name, sources, width, height, K, parameters): sources as tests/reproject_ref.py takes them, each with "offset": the elements
(points) of padding in front of it in its buffer, so that its pointer leaves the 16-byte bound; K = (fx, fy, cx, cy).  Every case runs into a
uint16 and into an int32 target."""
import numpy as np

import reproject_ref as R

DTYPES = (np.uint16, np.int32)
K_SMALL = (60.0, 61.5, 33.2, 22.1)                  # a 67 x 45 target
K_MID = (110.0, 108.0, 64.6, 38.3)                  # a 130 x 77 target
K_POW2 = (64.0, 64.0, 32.0, 16.0)                   # u and v exact for z = 1 and coordinates on multiples of 1 / 128
TARGETS = {"67x45": (67, 45, K_SMALL), "130x77": (130, 77, K_MID)}
VIS1 = dict(tol_mm=5, tol_permille=5, occl_radius=1, occl_min_front=2)
VIS2 = dict(tol_mm=5, tol_permille=5, occl_radius=2, occl_min_front=5)


def rigid(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """Rotations in degrees about x, y, z (applied in that order), then the translation in metres."""
    ax, ay, az = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


def src_frame(width, height, seed, near=600, far=1000):
    """A sloping background, a nearer block, 5 % holes, a negative value and a far outlier."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    d = far + xs + 2 * ys + rng.integers(-2, 3, size=(height, width))
    d = np.where((xs > width // 4) & (xs < width // 2) & (ys > height // 5) & (ys < 3 * height // 4), near + rng.integers(-2, 3, size=d.shape), d)
    d[rng.random(d.shape) < 0.05] = 0
    d[height // 2, 1] = -7
    d[1, width // 2] = 70000
    return d


def src_cloud(n, seed, bad=True):
    """n points in front of the camera, most inside a 60-degree cone; with `bad`, a few that are not finite, behind the camera or on its plane."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.4, 1.6, n)
    p = np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.5, 0.5, n) * z, z], 1).astype(np.float32)
    if bad and n >= 63:
        p[3] = (np.nan, 0, 1)
        p[7] = (0, np.inf, 1)
        p[11] = (0, 0, -np.inf)
        p[20] = (0.1, 0.1, 0.0)
        p[21] = (0.1, 0.1, -1.0)
        p[22] = (0.1, 0.1, np.nan)
        p[23] = (0.1, 0.1, np.inf)
        p[24] = (3e38, 0.1, 1.0)
        p[25] = (0.1, -3e38, 1e-30)
    return p


def _frame(d, K, T=None, offset=0, dtype=np.int32):
    s = R.frame(d, K, T)
    s["offset"], s["dtype"] = offset, dtype
    return s


def _cloud(p, T=None, offset=0):
    s = R.cloud(p, T)
    s["offset"] = offset
    return s


def border_points(width, height, K):
    """Points at z = 1 whose u and v are exactly the listed values: pixel centres, x.5, -0.5, width - 0.5 and beyond, in every combination."""
    fx, fy, cx, cy = K
    us = np.array([-4.0, -3.5, -3.0, -2.5, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 7.5, width - 2.0, width - 1.5, width - 1.0, width - 0.5, width, width + 0.5, width + 3.0])
    vs = np.array([-4.0, -3.5, -3.0, -2.5, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 7.5, height - 2.0, height - 1.5, height - 1.0, height - 0.5, height, height + 0.5, height + 3.0])
    uu, vv = np.meshgrid(us, vs)
    return np.stack([(uu.ravel() - cx) / fx, (vv.ravel() - cy) / fy, np.ones(uu.size)], 1).astype(np.float32)


def visibility_frame(width, height, n_front):
    """Background 1000 everywhere; around each probe pixel -- on both sides of the tile borders x = 63 | 64, 127 | 128 and y = 15 | 16, 31 | 32, 47 | 48, 63 | 64, and in
    the frame's corners -- n_front pixels at 900: ring 1 first (8 pixels), then ring 2."""
    d = np.full((height, width), 1000, np.int64)
    ring = [(dx, dy) for r in (1, 2) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if max(abs(dx), abs(dy)) == r]
    for px, py in [(63, 15), (64, 32), (20, 40), (127, 31), (128, 48), (100, 64), (0, 0), (width - 1, height - 1), (40, 63), (70, 16)]:
        if px >= width or py >= height:
            continue
        k = 0
        for dx, dy in ring:
            x, y = px + dx, py + dy
            if k < n_front and 0 <= x < width and 0 <= y < height:
                d[y, x] = 900
                k += 1
    return d


def cases():
    out = []
    # frames into frames: both targets, both source sizes, every splat, with and without the visibility stage; u16 and i32 sources alternate
    k = 0
    for tname, (tw, th, tk) in TARGETS.items():
        for sw, sh, sk in ((61, 37, (55.0, 56.0, 30.3, 18.2)), (130, 77, K_MID)):
            for splat in (1, 2, 3):
                T = rigid(3.0, -12.0, 2.0, (0.12, -0.03, 0.05))
                vis = (dict(), VIS1, VIS2)[k % 3]
                dt = (np.uint16, np.int32)[k % 2]
                d = src_frame(sw, sh, seed=k)
                if dt == np.uint16:
                    d = np.clip(d, 0, 65535)
                out.append((f"{tname}_from_{sw}x{sh}_s{splat}_{np.dtype(dt).name}", [_frame(d, sk, T, dtype=dt)], tw, th, tk, dict(vis, splat=splat, min_mm=100)))
                k += 1
    # pointers one element (one point) past a 16-byte bound: the partial first and last slot, the cloud's float-by-float loads
    d = np.clip(src_frame(61, 37, seed=50), 0, 65535)
    out.append(("offset_u16", [_frame(d, (55.0, 56.0, 30.3, 18.2), rigid(ry=5.0), 1, np.uint16)], 67, 45, K_SMALL, dict(splat=2)))
    out.append(("offset_i32", [_frame(src_frame(61, 37, seed=51), (55.0, 56.0, 30.3, 18.2), rigid(ry=-5.0), 1, np.int32)], 67, 45, K_SMALL, dict(splat=1)))
    out.append(("offset_cloud", [_cloud(src_cloud(1031, seed=52), rigid(rx=4.0), 1)], 130, 77, K_MID, dict(splat=2)))
    out.append(("tiny_frames", [_frame(np.array([[800]]), K_SMALL, None, 1, np.uint16), _frame(np.array([[700, 0, 900]]), K_SMALL, None, 1, np.int32),
                                _frame(np.arange(1, 10).reshape(3, 3) * 100, K_SMALL, None, 0, np.uint16)], 67, 45, K_SMALL, dict(splat=3)))
    # clouds around the lane, wavefront, workgroup and chunk sizes
    for n in (1, 63, 64, 65, 257, 4097):
        out.append((f"cloud_n{n}", [_cloud(src_cloud(n, seed=n), rigid(ry=8.0, t=(0.05, 0.0, 0.1)))], 130, 77, K_MID, dict(VIS1, splat=1 + n % 3)))
    # eight sources of mixed kinds and sizes in one call, two of them the same buffer
    same = _frame(np.clip(src_frame(130, 77, seed=61), 0, 65535), K_MID, rigid(ry=-10.0, t=(-0.1, 0, 0)), 0, np.uint16)
    eight = [_frame(src_frame(61, 37, seed=60), (55.0, 56.0, 30.3, 18.2), rigid(ry=10.0, t=(0.1, 0, 0)), 0, np.int32), same, _cloud(src_cloud(4097, seed=62)),
             _cloud(src_cloud(65, seed=63), rigid(rz=30.0), 1), _frame(np.clip(src_frame(61, 37, seed=64), 0, 65535), (55.0, 56.0, 30.3, 18.2), None, 1, np.uint16),
             dict(same, T=rigid(rx=6.0), shares=1), _cloud(src_cloud(257, seed=66), rigid(t=(0, 0, 0.3))), _frame(src_frame(130, 77, seed=67), K_MID, None, 1, np.int32)]
    out.append(("eight_sources", eight, 130, 77, K_MID, dict(VIS2, splat=2, min_mm=300, max_mm=1500)))
    out.append(("eight_sources_s1", eight, 67, 45, K_SMALL, dict(splat=1)))
    # 4096 samples of two sources on one pixel at one depth: the lower source index wins, whatever arrives first
    one = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (2048, 1))
    out.append(("tie_4096", [_cloud(one), _cloud(one)], 67, 45, K_POW2, dict(splat=1)))
    out.append(("tie_4096_nearer_later", [_cloud(one), _cloud(one), _cloud(np.array([[0.0, 0.0, 0.999]], np.float32))], 67, 45, K_POW2, dict(splat=3)))
    # u and v exactly on x.5, -0.5, width - 0.5: squares clipped at every border and corner
    for splat in (1, 2, 3):
        out.append((f"borders_s{splat}", [_cloud(border_points(67, 45, K_POW2))], 67, 45, K_POW2, dict(splat=splat)))
    # q.z zero and negative through the transform of a frame
    flat = np.full((37, 61), 500, np.int64)
    flat[::2] = 400
    flat[17:20], flat[7] = 900, 501
    out.append(("qz_zero_negative", [_frame(flat, (55.0, 56.0, 30.3, 18.2), rigid(t=(0, 0, -0.5)), 0, np.uint16)], 67, 45, K_SMALL, dict(splat=2)))
    # the gates: d at min_mm, max_mm and one beyond; 65535 and 65536; 2^28 - 1 and 2^28
    gate = np.array([[499, 500, 501, 0, 1999, 2000, 2001], [1, 65534, 65535, 65536, 65537, 2 ** 28 - 1, 2 ** 28], [2 ** 28 - 16, 2 ** 28 - 17, 2 ** 31 - 1, -1, 268435440, 100000, 16777217]])
    gk = (64.0, 64.0, 3.0, 1.0)
    out.append(("gate_min_max", [_frame(gate, gk)], 7, 3, gk, dict(splat=1, min_mm=500, max_mm=2000)))
    out.append(("gate_type", [_frame(gate, gk)], 7, 3, gk, dict(splat=1)))
    out.append(("gate_cloud", [_cloud(np.array([[0, 0, 0.4994], [0.02, 0, 0.4996], [0.04, 0, 65.5354], [0.06, 0, 65.5356], [0, 0.02, 268435.44], [0.02, 0.02, 268435.47], [0, 0, 3e38]], np.float32))],
                7, 3, gk, dict(splat=1, min_mm=500)))
    # visibility: Z[q] + tol one under and equal to Z[p]; front equal to and one under occl_min_front; radius 1 and 2 across tile borders
    for r, n_front in ((1, 3), (2, 11)):
        for tol_mm in (99, 100):
            for min_front in (n_front, n_front + 1):
                d = visibility_frame(130, 77, n_front)
                out.append((f"vis_r{r}_tol{tol_mm}_front{min_front}of{n_front}", [_frame(d, K_MID, None, 0, np.uint16)], 130, 77, K_MID,
                            dict(splat=1, tol_mm=tol_mm, occl_radius=r, occl_min_front=min_front)))
    out.append(("vis_permille", [_frame(visibility_frame(130, 77, 8), K_MID, None, 0, np.uint16)], 130, 77, K_MID, dict(splat=1, tol_permille=99, occl_radius=2, occl_min_front=8)))
    return out


def buffer_of(src):
    """The flat host buffer a source lies in -- `offset` elements (points) of padding, then the source -- and the element type's name."""
    if src["kind"] == "cloud":
        return np.concatenate([np.full(3 * src["offset"], 7.0, np.float32), src["data"].reshape(-1)])
    dt = src["dtype"]
    return np.concatenate([np.full(src["offset"], 77, dt), src["data"].astype(dt).reshape(-1)])


def ref_sources(sources):
    """The sources as the reference takes them: a frame's values as its dtype holds them."""
    return [dict(s, data=s["data"].astype(s["dtype"])) if s["kind"] == "frame" else s for s in sources]


def api_sources(api, sources, device):
    """The sources as pose_refine_amd.api takes them, on the device (DeviceVectors; a source with `shares` uses the buffer of that earlier source) or
    on the host."""
    made, bufs = [], []
    for s in sources:
        buf = bufs[s["shares"]] if "shares" in s else (api.DeviceVector.from_host(buffer_of(s)) if device else buffer_of(s))
        bufs.append(buf)
        if s["kind"] == "cloud":
            made.append(api.ReprojectSource.cloud(buf, s["T"], offset_points=s["offset"]))
        else:
            h, w = s["data"].shape
            made.append(api.ReprojectSource.frame(buf, w, h, (s["K"][0], 0, s["K"][2], 0, s["K"][1], s["K"][3], 0, 0, 1), s["T"], offset_elems=s["offset"]))
    return made
