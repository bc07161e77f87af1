"""The frames of the scene-segment tests, shared by the host and the GPU tests: every case is (name, depth as int64[h, w], parameters, the depth
types it is run in), and its reference (tests/segments_ref.py) is computed once per process."""
import functools
from collections import namedtuple

import numpy as np

import segments_ref as R

Case = namedtuple("Case", "name depth kw dtypes")
BOTH, I32 = (np.uint16, np.int32), (np.int32,)
SIZES = [(67, 45), (130, 77), (200, 150)]            # no plausible tile size divides them
THIN = [(1, 1), (1, 97), (97, 1)]
JUMP = 10
I32_MAX = 2 ** 31 - 1


def spiral_mask(w, h):
    """a one-pixel-wide spiral with one-pixel gaps from the top left corner inwards"""
    m = np.zeros((h, w), bool)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = True

    def free(px, py):
        return 0 <= px < w and 0 <= py < h and not m[py, px]

    while True:
        for _ in range(2):
            ahead_painted = 0 <= x + 2 * dx < w and 0 <= y + 2 * dy < h and m[y + 2 * dy, x + 2 * dx]
            ok = free(x + dx, y + dy) and not ahead_painted
            if ok:
                break
            dx, dy = -dy, dx
        if not ok:
            return m
        x, y = x + dx, y + dy
        m[y, x] = True


def comb_mask(w, h):
    """teeth in every other column over the full height, joined in the last row only"""
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    m[h - 1, :] = True
    return m


def noise(w, h, seed, holes=0.3, lo=500, hi=540):
    rng = np.random.default_rng(seed)
    d = rng.integers(lo, hi, (h, w), dtype=np.int64)
    d[rng.random((h, w)) < holes] = 0
    return d


def squares(w, h, sizes, depth=700):
    """squares of the given sides, one pixel apart at least, left to right and wrapped"""
    d = np.zeros((h, w), np.int64)
    x = y = 1
    row_h = 0
    for s in sizes:
        if x + s + 1 > w:
            x, y, row_h = 1, y + row_h + 1, 0
        assert y + s < h
        d[y:y + s, x:x + s] = depth
        x, row_h = x + s + 1, max(row_h, s)
    return d


def _cases():
    out = []
    for w, h in SIZES:
        tag = f"{w}x{h}"
        sp = spiral_mask(w, h)
        kw1 = dict(jump_mm=JUMP, min_pixels=1, max_segments=64)
        out.append(Case(f"spiral_{tag}", np.where(sp, 900, 0).astype(np.int64), kw1, BOTH))
        out.append(Case(f"spirals_interleaved_{tag}", np.where(sp, 900, 900 + JUMP + 1).astype(np.int64), kw1, BOTH))
        out.append(Case(f"noise_{tag}", noise(w, h, seed=w), dict(jump_mm=JUMP, min_pixels=1, max_segments=R.SEGMENT_MAX), BOTH))
        if (w, h) == SIZES[2]:
            continue
        cm = comb_mask(w, h)
        out.append(Case(f"comb_{tag}", np.where(cm, 800, 0).astype(np.int64), kw1, BOTH))
        out.append(Case(f"u_shapes_{tag}", np.where(comb_mask(h, w).T, 800, 0).astype(np.int64), kw1, BOTH))
        # two combs into each other without a gap: teeth from the top at one depth, from the bottom at another
        inter = np.full((h, w), 800 + 5 * JUMP, np.int64)           # the bottom comb: the last row and the odd columns
        inter[:h - 1, ::2] = 800                                   # the top comb: the first row and the even columns
        inter[0, :] = 800
        out.append(Case(f"combs_interlocked_{tag}", inter, kw1, BOTH))
        stairs = np.broadcast_to(100 + JUMP * np.arange(w, dtype=np.int64), (h, w)).copy()
        out.append(Case(f"staircase_{tag}", stairs, kw1, BOTH))
        cut = stairs.copy()
        cut[:, w // 2:] += 1                                      # one step of jump + 1 in the middle
        out.append(Case(f"staircase_cut_{tag}", cut, kw1, BOTH))
        diag = (100 + JUMP * (np.arange(w, dtype=np.int64)[None, :] + np.arange(h, dtype=np.int64)[:, None]))
        out.append(Case(f"staircase_diagonal_{tag}", diag, kw1, BOTH))
        out.append(Case(f"noise_few_{tag}", noise(w, h, seed=h), dict(jump_mm=JUMP, min_pixels=3, max_segments=5), BOTH))
        out.append(Case(f"empty_{tag}", np.zeros((h, w), np.int64), kw1, BOTH))
    for w, h in THIN:
        out.append(Case(f"noise_{w}x{h}", noise(w, h, seed=w + h, holes=0.2, lo=500, hi=530), dict(jump_mm=JUMP, min_pixels=1, max_segments=64), BOTH))
    out.append(Case("one_pixel_unmeasured", np.zeros((1, 1), np.int64), dict(jump_mm=JUMP, min_pixels=1, max_segments=1), BOTH))
    # the tie rule: four squares of 100 pixels and two of 64; min_pixels exactly at a size and one above
    sq = squares(67, 45, [10, 8, 10, 10, 8, 10, 6])
    for mp in (1, 64, 65, 100, 101):
        out.append(Case(f"squares_min{mp}", sq, dict(jump_mm=JUMP, min_pixels=mp, max_segments=64), BOTH))
    out.append(Case("squares_max3", sq, dict(jump_mm=JUMP, min_pixels=1, max_segments=3), BOTH))
    out.append(Case("squares_jump0", sq, dict(jump_mm=0, min_pixels=1, max_segments=64), BOTH))
    # one constant frame: one component, the largest sums a uint16 frame of this size has
    out.append(Case("constant_640x480", np.full((480, 640), 65535, np.int64), dict(jump_mm=0, min_pixels=256, max_segments=64), BOTH))
    # int32 alone: negative values are not measured; 1 next to 2^31 - 1 must not overflow, and at jump 2^31 - 1 the two ARE linked
    ext = noise(67, 45, seed=5).astype(np.int64)
    ext[::3, ::2] = -7
    ext[1::4, 1::3] = -(2 ** 31)
    ext[10:20, 10:40:2] = 1
    ext[10:20, 11:40:2] = I32_MAX
    ext[30:35, 5:60] = I32_MAX
    ext[35:40, 5:60] = I32_MAX - JUMP
    for j in (JUMP, I32_MAX - 2, I32_MAX):
        out.append(Case(f"int32_extremes_jump{j}", ext, dict(jump_mm=j, min_pixels=1, max_segments=R.SEGMENT_MAX), I32))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.depth.size <= 130 * 77]      # the second formulation is run on these

# over PR_SEGMENT_MAX_ROOTS: 370 x 356 / 2 = 65 860 pixels of each of two depths, no two of one depth 4-adjacent -> 131 720 components of 1 pixel
CHECKERBOARD = np.where((np.arange(356)[:, None] + np.arange(370)[None, :]) % 2 == 0, 600, 600 + JUMP + 1).astype(np.int64)
CHECKERBOARD_KW = dict(jump_mm=JUMP, min_pixels=1, max_segments=64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's reference, once; callers leave it unchanged"""
    c = BY_NAME[name]
    ref = R.scene_segments(c.depth, **c.kw)
    for v in (ref["segments"], ref["labels"], ref["roots"]):
        v.setflags(write=False)
    return ref


def assert_same(got, ref, what=""):
    """got: (segments, labels[h, w], roots[h, w], counts) of an entry point"""
    segs, labels, roots, counts = got
    assert tuple(counts) == tuple(ref["counts"]), what
    assert roots.dtype == np.uint32 and roots.tobytes() == ref["roots"].tobytes(), what
    assert labels.dtype == np.uint16 and labels.tobytes() == ref["labels"].tobytes(), what
    assert segs.dtype.itemsize == 64 and segs.tobytes() == ref["segments"].tobytes(), what


# ---- the scenario: two objects on the 25-degree table of tests/test_planes_gpu.py ----------------------------------------------------------------
TABLE_TILT_DEG = 25.0


def blob_mesh_and_pose():
    """the bumped blob of tests/test_ppf_multi_gpu.py restated (768 triangles, stretched differently along every axis) and its pose: left of and
    above obj_06 in the image"""
    from pose_refine_amd import synth
    tris = (synth.uv_sphere_mesh(24, 16).astype(np.float64) * [1.0, 0.7, 0.45]).astype(np.float32)
    q, _ = np.linalg.qr(np.random.default_rng(21).normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return tris, synth.pose_matrix(q.astype(np.float32), np.array([-150.0, -50.0, 400.0], np.float32))


def four_adjacent(a, b):
    """a pixel of mask a has a 4-neighbour (or itself) in mask b"""
    g = b.copy()
    g[:, 1:] |= b[:, :-1]
    g[:, :-1] |= b[:, 1:]
    g[1:, :] |= b[:-1, :]
    g[:-1, :] |= b[1:, :]
    return bool((a & g).any())


def two_object_frame(d_obj, d_blob):
    """(depth uint16, mask of obj_06, mask of the blob): the two renders over the analytic table -- the plane z = const turned 25 degrees about the
    camera's x axis, pushed back until it lies 5 mm (rounded up to a whole mm of offset) behind the object pixel nearest to it"""
    import math

    import planes_cases as PC
    from pose_refine_amd import synth
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    m_obj, m_blob = d_obj > 0, d_blob > 0
    assert m_obj.any() and m_blob.any() and not four_adjacent(m_obj, m_blob)       # two objects whose masks do not touch
    both = m_obj | m_blob
    render = np.where(m_obj, d_obj, d_blob)
    n = PC.tilted(TABLE_TILT_DEG)
    den = PC.rays(W, H, K) @ n
    d = -(math.ceil((render[both].astype(np.float64) * np.abs(den[both])).max()) + 5.0)
    zp = PC.plane_depth(W, H, K, n, d)
    assert (zp[both] > render[both]).all() and zp.max() < 65535
    return np.where(both, render, np.rint(zp)).astype(np.uint16), m_obj, m_blob


def largest_share(labels, mask):
    """(label, share): the segment with the most pixels inside mask and the share of the mask it holds"""
    inside = labels[mask]
    inside = inside[(inside != 0) & (inside != R.SEGMENT_DROPPED)]
    if len(inside) == 0:
        return 0, 0.0
    ids, n = np.unique(inside, return_counts=True)
    k = int(np.argmax(n))
    return int(ids[k]), float(n[k]) / float(mask.sum())
