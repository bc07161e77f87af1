"""Reprojection restated in numpy from the text of include/pose_refine.h ("reprojection"): float32 arrays up to the footprint, int64 from there on,
the z-buffer by np.minimum.at over the samples.  The reference the host twin and the device are held to, byte for byte.  Nothing here looks at
pose_refine_amd/csrc/reproject.h.

A source is a dict: kind "frame" (data: int array[height, width], K: (fx, fy, cx, cy)) or "cloud" (data: float32[n, 3]), and T (4 x 4; default
the identity)."""
import numpy as np

HIDDEN, NONE = 254, 255
MAX_DEPTH = 2 ** 28 - 1
_NO_KEY = np.int64(0xFFFFFFFF)
_F = np.float32

PARAM_DEFAULTS = dict(splat=1, min_mm=0, max_mm=0, tol_mm=0, tol_permille=0, occl_radius=0, occl_min_front=0)


def frame(data, K, T=None):
    return dict(kind="frame", data=np.asarray(data), K=tuple(K), T=np.eye(4) if T is None else T)


def cloud(data, T=None):
    return dict(kind="cloud", data=np.asarray(data, np.float32).reshape(-1, 3), T=np.eye(4) if T is None else T)


def pinhole(K):
    """(fx, fy, cx, cy) of a 3 x 3 matrix."""
    k = np.asarray(K, np.float32).reshape(-1)
    return float(k[0]), float(k[4]), float(k[2]), float(k[5])


def tol(d, p):
    return np.int64(p["tol_mm"]) + d * np.int64(p["tol_permille"]) // 1000


def _shift(a, dx, dy):
    """a at (x + dx, y + dy); 0 outside the frame."""
    h, w = a.shape
    r = max(abs(dx), abs(dy))
    pad = np.pad(a, r, constant_values=0)
    return pad[r + dy:r + dy + h, r + dx:r + dx + w]


def samples_of(src):
    """(points float32[n, 3] of the source's samples that reach the transform, the number of samples, those counted `range` before it)"""
    if src["kind"] == "cloud":
        pts = src["data"]
        return pts, len(pts), 0
    d = src["data"].astype(np.int64)
    d0 = np.where(d > 0, d, 0)
    ys, xs = np.nonzero(d0)
    dd = d0[ys, xs]
    far = dd > MAX_DEPTH
    ys, xs, dd = ys[~far], xs[~far], dd[~far]
    fx, fy, cx, cy = (_F(v) for v in src["K"])
    z = dd.astype(_F) / _F(1000.0)
    pts = np.stack([(xs.astype(_F) - cx) / fx * z, (ys.astype(_F) - cy) / fy * z, z], 1)
    return pts, len(far), int(far.sum())


def reproject(sources, width, height, K, dtype, params):
    """(out of dtype[height, width], source uint8[height, width], counts) -- counts as pose_refine_amd.api.depth_reproject returns them."""
    p = dict(PARAM_DEFAULTS, **params)
    fx, fy, cx, cy = (_F(v) for v in K)
    s = int(p["splat"])
    lo = max(1, p["min_mm"])
    hi = min(MAX_DEPTH, 65535 if np.dtype(dtype) == np.uint16 else MAX_DEPTH, p["max_mm"] if p["max_mm"] else MAX_DEPTH)
    h = _F(0.5) * _F(2 - s)
    keys = np.full(width * height, _NO_KEY, np.int64)
    per = []
    with np.errstate(all="ignore"):
        for i, src in enumerate(sources):
            pts, n_samples, n_range = samples_of(src)
            T = np.asarray(src["T"], _F).reshape(4, 4)
            px, py, pz = pts[:, 0], pts[:, 1], pts[:, 2]
            q = [((T[c, 0] * px + T[c, 1] * py) + T[c, 2] * pz) + T[c, 3] for c in range(3)]
            ok = np.isfinite(pts).all(1) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2]) & (q[2] > 0)
            n_invalid = int((~ok).sum())
            qx, qy, qz = (c[ok] for c in q)
            df = np.floor(qz * _F(1000.0) + _F(0.5)).astype(np.float64)
            gate = (df >= lo) & (df <= hi)
            n_range += int((~gate).sum())
            qx, qy, qz, d = qx[gate], qy[gate], qz[gate], df[gate].astype(np.int64)
            u, v = qx / qz * fx + cx, qy / qz * fy + cy
            x0f, y0f = np.floor(u + h), np.floor(v + h)
            inside = (x0f > _F(-4.0)) & (x0f < _F(width)) & (y0f > _F(-4.0)) & (y0f < _F(height))
            x0, y0, key = x0f[inside].astype(np.int64), y0f[inside].astype(np.int64), (d[inside] << 3) | i
            hit = np.zeros(len(x0), bool)
            for dy in range(s):
                for dx in range(s):
                    x, y = x0 + dx, y0 + dy
                    m = (x >= 0) & (x < width) & (y >= 0) & (y < height)
                    np.minimum.at(keys, (y * width + x)[m], key[m])
                    hit |= m
            n_outside = int((~inside).sum()) + int((~hit).sum())
            per.append(dict(samples=n_samples, invalid=n_invalid, range=n_range, outside=n_outside, drawn=n_samples - n_invalid - n_range - n_outside, won=0))
    keys = keys.reshape(height, width)
    Z = np.where(keys == _NO_KEY, 0, keys >> 3)
    S = keys & 7
    hidden = np.zeros(Z.shape, bool)
    r = p["occl_radius"]
    if p["occl_min_front"] > 0:
        front = np.zeros_like(Z)
        t = tol(Z, p)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx or dy:
                    q = _shift(Z, dx, dy)
                    front += (q != 0) & (q + t < Z)
        hidden = (Z != 0) & (front >= p["occl_min_front"])
    kept = (Z != 0) & ~hidden
    out = np.where(kept, Z, 0).astype(dtype)
    source = np.where(kept, S, np.where(hidden, HIDDEN, NONE)).astype(np.uint8)
    for i, rec in enumerate(per):
        rec["won"] = int((source == i).sum())
    return out, source, dict(sources=per, covered=int((Z != 0).sum()), hidden=int(hidden.sum()), kept=int(kept.sum()))


def keys_of(out, source):
    """The per-pixel key (d << 3) | s of a result without hidden pixels; 2^32 - 1 where nothing landed."""
    return np.where(out != 0, (out.astype(np.int64) << 3) | (source.astype(np.int64) & 7), _NO_KEY)


# ---- the analytic scene of the property test ----------------------------------------------------------------------------------------------
def rot_y(deg):
    a = np.deg2rad(deg)
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return R
