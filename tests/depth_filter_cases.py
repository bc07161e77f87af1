"""The small frames of the depth-conditioning tests (test_depth_filter_host.py, test_depth_filter_gpu.py): the smallest shapes at which the
stencil, its tiles (64 x 16), its clipped windows, the selection and the fuse's vector path can still go wrong.  A filter case is (name, depth
int64[height, width], parameters); a test casts it to uint16 and int32 where the values fit (`dtypes_of`)."""
import numpy as np

I32_MAX = 2 ** 31 - 1
ALL = dict(min_mm=100, max_mm=5000, tol_mm=6, tol_permille=5, fly_min_support=3, radius=1, fill_min=5)


def dtypes_of(depth):
    """The depth types a case runs in: both, unless a value does not fit uint16 (negative values are an int32 matter)."""
    return [np.int32] if (depth.min() < 0 or depth.max() > 65535) else [np.uint16, np.int32]


def tiled_frame(width, height, seed):
    """A background that slopes, a foreground block whose borders lie exactly on x = 63 | 64, x = 127 | 128, y = 15 | 16 and the later tile rows,
    flying pixels on those borders, holes and one-pixel lines across them, and the same on the frame's corners and borders."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    d = 1000 + xs + 2 * ys + rng.integers(-2, 3, size=(height, width))
    fg = (xs >= 20) & (xs < 64) & (ys >= 5) & (ys < 32)                        # right edge between columns 63 | 64, lower edge between rows 31 | 32
    fg |= (xs >= 64) & (xs < 128) & (ys >= 16) & (ys < 48)                     # upper edge between rows 15 | 16, right edge 127 | 128, lower 47 | 48
    d = np.where(fg, 600 + rng.integers(-2, 3, size=d.shape), d)
    for x, y in [(63, 10), (64, 10), (63, 15), (64, 16), (63, 16), (64, 15), (127, 20), (128, 20), (127, 47), (100, 15), (100, 16), (90, 47), (90, 48), (30, 31), (30, 32)]:
        if x < width and y < height:
            d[y, x] = 800                                                      # between foreground and background: flying
    for x, y in [(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, 0), (0, height // 2), (width - 1, height // 2), (width // 2, height - 1)]:
        d[y, x] = 800 if (x + y) % 2 else 0                                    # corners and borders: flying pixels and holes where the window is clipped
    for x, y in [(62, 14), (63, 15), (64, 16), (65, 17), (63, 31), (64, 32), (127, 33), (128, 33), (5, 15), (5, 16), (1, 1), (width - 2, height - 2)]:
        if x < width and y < height:
            d[y, x] = 0                                                        # holes on both sides of the tile corners
    if height > 34 and width > 66:
        d[33:36, 62:66] = 0                                                    # a block of holes across x = 63 | 64: its middle has too few neighbours to fill at radius 1
    for x, y, v in [(3, 2, 50), (64, 17, 6000), (63, 17, 40), (width - 1, 3, 9000), (10, height - 1, 99)]:
        d[y, x] = v                                                            # outside the gate of ALL, with good neighbours all around
    d[min(40, height - 1), :] = 700                                          # a one-pixel line across every tile column ...
    d[:, min(66, width - 1)] = 700                                             # ... and one across every tile row, next to a tile border
    holes = rng.random(d.shape) < 0.03
    d[holes] = 0
    return d


def filter_cases():
    cases = []
    # degenerate frames
    cases.append(("1x1", np.array([[1000]]), ALL))
    cases.append(("1x1_hole", np.array([[0]]), ALL))
    cases.append(("1x1_no_fly", np.array([[1000]]), dict(ALL, fly_min_support=0)))
    cases.append(("1x7", np.array([[1000, 1001, 0, 1002, 1500, 1003, 1001]]), dict(ALL, fly_min_support=1, fill_min=1)))
    cases.append(("7x1", np.array([[1000, 1001, 0, 1002, 1500, 1003, 1001]]).T.copy(), dict(ALL, fly_min_support=2, fill_min=2)))
    # frames that cross tile borders: each stage alone, all together, both radii, the support and fill thresholds
    for w, h in ((67, 45), (130, 77)):
        d = tiled_frame(w, h, seed=w)
        variants = {
            "gate": dict(min_mm=650, max_mm=1100),
            "gate_no_max": dict(min_mm=650, max_mm=0),
            "gate_all": dict(min_mm=3000, max_mm=4000, fly_min_support=3, radius=2, fill_min=3, tol_mm=6),
            "fly1": dict(tol_mm=6, tol_permille=5, fly_min_support=1),
            "fly3": dict(tol_mm=6, tol_permille=5, fly_min_support=3),
            "fly8": dict(tol_mm=6, tol_permille=5, fly_min_support=8),
            "median_r1": dict(tol_mm=6, tol_permille=5, radius=1),
            "median_r2": dict(tol_mm=6, tol_permille=5, radius=2),
            "median_r2_wide": dict(tol_mm=500, radius=2),                      # a tolerance that mixes across the jump: 25 candidates everywhere inside
            "fill_r1_min1": dict(tol_mm=6, tol_permille=5, radius=1, fill_min=1),
            "fill_r1_min8": dict(tol_mm=6, tol_permille=5, radius=1, fill_min=8),
            "fill_r2_min1": dict(tol_mm=6, tol_permille=5, radius=2, fill_min=1),
            "fill_r2_min24": dict(tol_mm=6, tol_permille=5, radius=2, fill_min=24),
            "all_r1": ALL,
            "all_r2": dict(ALL, radius=2, fill_min=13),
            "none": dict(),
        }
        for name, p in variants.items():
            cases.append((f"{w}x{h}_{name}", d, p))
    # median order: equal values, an even count (the lower median is not the upper), candidates exactly at tol and at tol + 1
    cases.append(("equal_5x5", np.full((5, 5), 1234), dict(tol_mm=0, radius=2, fill_min=1)))
    even = np.array([[10, 20, 30], [40, 25, 0], [50, 60, 70]]) + 1000           # the centre's window: 8 values, lower median 1030 and upper 1040
    cases.append(("even_3x3", even, dict(tol_mm=100, radius=1)))
    cases.append(("even_3x3_r2", even, dict(tol_mm=100, radius=2, fill_min=8)))
    at_tol = np.array([[1000 - 10, 1000 + 10, 1000 - 11], [1000 + 11, 1000, 1000 + 10], [1000 - 10, 1000 + 11, 1000 - 11]])
    cases.append(("at_tol_median", at_tol, dict(tol_mm=5, tol_permille=5, radius=1)))                     # tol(1000) = 10
    cases.append(("at_tol_support4", at_tol, dict(tol_mm=5, tol_permille=5, fly_min_support=4)))          # the centre has exactly four within 10
    cases.append(("at_tol_support5", at_tol, dict(tol_mm=5, tol_permille=5, fly_min_support=5)))
    ties = np.array([[7, 7, 9, 9, 7], [9, 7, 7, 9, 9], [7, 9, 8, 7, 9], [9, 9, 7, 7, 7], [7, 9, 9, 7, 0]]) + 500
    cases.append(("ties_r2", ties, dict(tol_mm=1, radius=2, fill_min=12)))
    cases.append(("ties_r1", ties, dict(tol_mm=1, radius=1, fill_min=3)))
    # a hole between half foreground and half background: |C| = 8, m = 600, |A| = 4
    half = np.array([[600, 600, 1000], [600, 0, 1000], [600, 1000, 1000]])
    cases.append(("half_fill5", half, dict(tol_mm=10, radius=1, fill_min=5)))    # the A test refuses it
    cases.append(("half_fill4", half, dict(tol_mm=10, radius=1, fill_min=4)))    # ... and lets it pass
    # a gated pixel and a flying pixel inside a full ring of good neighbours stay 0
    ring = np.full((5, 5), 1000)
    gated, fly = ring.copy(), ring.copy()
    gated[2, 2], fly[2, 2] = 50, 800
    cases.append(("gated_in_ring", gated, dict(ALL, fill_min=1)))
    cases.append(("flying_in_ring", fly, dict(ALL, fill_min=1)))
    cases.append(("flying_in_ring_r2", fly, dict(ALL, radius=2, fill_min=1)))
    # values: the largest uint16; int32: negative values, 2^31 - 1, differences beyond 2^31 as signed words, tol_permille = 1000 at large depth
    big16 = np.array([[65535, 65535, 65530], [65535, 0, 65531], [1, 65535, 65535]])
    cases.append(("u16_max", big16, dict(tol_mm=5, fly_min_support=2, radius=1, fill_min=4)))
    cases.append(("u16_max_permille", big16, dict(tol_permille=1000, fly_min_support=2, radius=1, fill_min=4)))
    big32 = np.array([[I32_MAX, -5, I32_MAX - 3, 1], [-(2 ** 31), I32_MAX, 0, I32_MAX - 1], [2, I32_MAX - 2, I32_MAX, -1], [I32_MAX, 1, 3, I32_MAX]])
    cases.append(("i32_extremes", big32, dict(tol_mm=3, fly_min_support=1, radius=1, fill_min=2)))
    cases.append(("i32_extremes_r2", big32, dict(tol_mm=I32_MAX, tol_permille=1000, fly_min_support=3, radius=2, fill_min=3)))
    cases.append(("i32_permille", big32, dict(tol_permille=1000, min_mm=2, max_mm=I32_MAX, fly_min_support=2, radius=2, fill_min=1)))
    cases.append(("i32_gate_top", big32, dict(min_mm=I32_MAX, max_mm=I32_MAX, radius=1, fill_min=1)))
    return cases


def fuse_frames(n_frames, n_px, seed, high=3000):
    """n_frames x n_px depths: pixels measured in no, one, some or all frames, with ties."""
    rng = np.random.default_rng(seed)
    base = rng.integers(500, high, size=n_px)
    f = base[None] + rng.integers(-2, 3, size=(n_frames, n_px))              # a span of five values: ties are common
    seen = rng.random((n_frames, n_px)) < rng.choice([0.0, 0.15, 0.6, 1.0], size=n_px)[None]
    return np.where(seen, f, 0)


def fuse_cases():
    """(name, frames int64[n_frames, n_px], min_frames)"""
    cases = []
    for n in (1, 2, 5, 8):
        for n_px in (1, 61, 203, 1031):                                        # no multiple of 8 or 64; more than one workgroup; a tail behind the 16-byte groups
            for min_frames in sorted({1, n}):
                cases.append((f"n{n}_px{n_px}_min{min_frames}", fuse_frames(n, n_px, seed=100 * n + n_px), min_frames))
    cases.append(("n8_px512_min3", fuse_frames(8, 512, seed=7), 3))             # whole 16-byte groups only
    # every pattern of two values over eight frames (the sorting network, by the zero-one principle), and of measured / not measured
    bits = (np.arange(256)[None] >> np.arange(8)[:, None]) & 1
    cases.append(("zero_one", np.where(bits, 9, 5), 1))
    cases.append(("presence", np.where(bits, 700 + np.arange(8)[:, None], 0), 1))
    cases.append(("presence_min4", np.where(bits, 700 - np.arange(8)[:, None], 0), 4))
    ext = fuse_frames(5, 77, seed=3)
    ext[:, :5] = [[I32_MAX, -1, 1, I32_MAX, 0], [I32_MAX - 1, -(2 ** 31), 0, 1, 0], [1, 5, 0, I32_MAX, -7], [I32_MAX, 0, 3, 2, 0], [2, 0, I32_MAX, 2, -1]]
    cases.append(("i32_extremes", ext, 2))
    top = fuse_frames(3, 40, seed=4)
    top[:, :3] = [[65535, 65535, 1], [65535, 0, 65535], [1, 65534, 0]]
    cases.append(("u16_max", top, 1))
    return cases
