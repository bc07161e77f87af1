"""Depth conditioning restated in numpy from the text of include/pose_refine.h ("depth conditioning"), in int64: the reference the host twins and
the device are held to, byte for byte.  Nothing here looks at pose_refine_amd/csrc/depth_filter.h."""
import numpy as np

UNMEASURED, KEPT, SMOOTHED, GATED, FLYING, FILLED = range(6)
_BIG = np.int64(1) << 40                         # above every depth: where a masked-out candidate sorts


def depth_of(depth):
    """D0: the depth as an unsigned value; a non-positive int32 is 0."""
    d = np.asarray(depth).astype(np.int64)
    return np.where(d > 0, d, 0)


def tol(d, p):
    return np.int64(p["tol_mm"]) + d * np.int64(p["tol_permille"]) // 1000


def _shift(a, dx, dy):
    """a at (x + dx, y + dy); 0 outside the frame."""
    h, w = a.shape
    r = max(abs(dx), abs(dy))
    pad = np.pad(a, r, constant_values=0)
    return pad[r + dy:r + dy + h, r + dx:r + dx + w]


def lower_median(values, mask):
    """Per pixel: element (k - 1) // 2 of the ascending order of the k values whose mask is set (axis 0); 0 where k == 0."""
    k = mask.sum(axis=0)
    order = np.sort(np.where(mask, values, _BIG), axis=0)
    pick = np.take_along_axis(order, np.maximum((k - 1) // 2, 0)[None], axis=0)[0]
    return np.where(k > 0, pick, 0), k


PARAM_DEFAULTS = dict(min_mm=0, max_mm=0, tol_mm=0, tol_permille=0, fly_min_support=0, radius=0, fill_min=0)


def depth_filter(depth, params):
    """(out of the depth's dtype, flags uint8, counts: six ints) of a height x width depth image."""
    p = dict(PARAM_DEFAULTS, **params)
    depth = np.asarray(depth)
    D0 = depth_of(depth)
    G = np.where((D0 != 0) & (D0 >= p["min_mm"]) & ((p["max_mm"] == 0) | (D0 <= p["max_mm"])), D0, 0)
    tG = tol(G, p)
    support = np.zeros_like(G)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                q = _shift(G, dx, dy)
                support += (q != 0) & (np.abs(q - G) <= tG)
    F = np.where((G != 0) & ((p["fly_min_support"] == 0) | (support >= p["fly_min_support"])), G, 0)
    r = p["radius"]
    out = F.copy()
    if r > 0:
        Q = np.stack([_shift(F, dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
        med, _ = lower_median(Q, (Q != 0) & (np.abs(Q - F[None]) <= tol(F, p)[None]))
        out = np.where(F != 0, med, 0)
        if p["fill_min"] > 0:
            in_c = Q != 0
            m, n_c = lower_median(Q, in_c)
            n_a = (in_c & (np.abs(Q - m[None]) <= tol(m, p)[None])).sum(axis=0)
            out = np.where((D0 == 0) & (n_c >= p["fill_min"]) & (n_a >= p["fill_min"]), m, out)
    flags = np.full(D0.shape, 255, np.uint8)
    flags[(D0 == 0) & (out == 0)] = UNMEASURED
    flags[(D0 == 0) & (out != 0)] = FILLED
    flags[(D0 != 0) & (G == 0)] = GATED
    flags[(G != 0) & (F == 0)] = FLYING
    flags[(F != 0) & (out == D0)] = KEPT
    flags[(F != 0) & (out != D0)] = SMOOTHED
    assert flags.max() <= FILLED and not (out[(flags == GATED) | (flags == FLYING)]).any() and (out[F != 0] != 0).all()
    return out.astype(depth.dtype), flags, tuple(int((flags == c).sum()) for c in range(6))


def depth_fuse(frames, min_frames):
    """(out of the frames' dtype, count uint8) of same-shaped depth arrays of one view."""
    D = np.stack([depth_of(f) for f in frames])
    m, k = lower_median(D, D != 0)
    return np.where(k >= min_frames, m, 0).astype(np.asarray(frames[0]).dtype), k.astype(np.uint8)


# ---- the analytic scene of the property tests --------------------------------------------------------------------------------------------
def clean_scene(width=160, height=120, f=150.0):
    """Nearest hit, rounded to integer mm, of: a tilted plane through depth 900, a sphere of radius 70 at (-40, 10, 600) and a fronto-parallel plate
    at z = 650.  Pixel (x, y) is the ray ((x - cx) / f, (y - cy) / f, 1) with the principal point at the frame's centre; every length but f is in
    mm and does not scale with the frame."""
    xs = (np.arange(width, dtype=np.float64) - (width - 1) / 2.0) / f
    ys = (np.arange(height, dtype=np.float64) - (height - 1) / 2.0) / f
    rx, ry = np.meshgrid(xs, ys)
    n = np.array([0.3, 0.4, 0.866])
    n /= np.linalg.norm(n)
    z = 900.0 * n[2] / (rx * n[0] + ry * n[1] + n[2])                          # the plane through (0, 0, 900)
    c = np.array([-40.0, 10.0, 600.0])
    a = rx * rx + ry * ry + 1.0
    b = rx * c[0] + ry * c[1] + c[2]
    disc = b * b - a * (c @ c - 70.0 ** 2)
    zs = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    plate = np.where((np.abs(650.0 * rx - 120.0) < 50.0) & (np.abs(650.0 * ry + 30.0) < 35.0), 650.0, np.inf)
    return np.rint(np.minimum(np.minimum(z, zs), plate)).astype(np.int64)


def corrupt(clean, seed, hole_block=((40, 43), (50, 53))):
    """(frame int64, flying mask, hole mask) of the corruption recipe: noise in -2 .. 2, flying pixels at depth jumps of more than 60, 2 % holes and
    one 3 x 3 hole."""
    rng = np.random.default_rng(seed)
    h, w = clean.shape
    frame = clean + rng.integers(-2, 3, size=clean.shape)
    flying = np.zeros(clean.shape, bool)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        nb = _shift(clean, dx, dy)
        jump = (nb != 0) & (np.abs(clean - nb) > 60)
        hit = jump & (rng.random(clean.shape) < 0.5)
        lo, hi = np.minimum(clean, nb) + 20, np.maximum(clean, nb) - 20
        val = rng.integers(lo, np.maximum(hi, lo) + 1)
        frame = np.where(hit, val, frame)
        flying |= hit
    holes = ~flying & (rng.random(clean.shape) < 0.02)
    (y0, y1), (x0, x1) = hole_block
    holes[y0:y1, x0:x1] = True
    flying &= ~holes
    frame = np.where(holes, 0, frame)
    return frame, flying, holes
