"""Scene segments restated from the text of include/pose_refine.h alone, in numpy and plain Python: a flood fill over the link relation, then the
records and the order.  It shares no code with the library; tests hold pr_scene_segments_host and pr_scene_segments_dev to it byte for byte."""
import numpy as np

SEGMENT_MAX, SEGMENT_MAX_ROOTS, SEGMENT_DROPPED = 4096, 65536, 65535
NO_ROOT = 0xFFFFFFFF
RECORD = np.dtype([("root", "<u4"), ("pixels", "<u4"), ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2"), ("depth_min", "<u4"), ("depth_max", "<u4"),
                   ("sum_x", "<u8"), ("sum_y", "<u8"), ("sum_depth", "<u8"), ("reserved", "<u8", (2,))])


class Refused(Exception):
    """what the library answers with PR_ERR_INVALID"""


def check_params(jump_mm, min_pixels, max_segments):
    if min_pixels == 0 or not 1 <= max_segments <= SEGMENT_MAX or jump_mm > 2 ** 31 - 1:
        raise Refused("parameters")


def check_frame(width, height):
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and width * height <= 2 ** 26):
        raise Refused("frame")


def links(depth, jump_mm):
    """(right[h, w], down[h, w]): pixel (y, x) is linked to (y, x + 1) / (y + 1, x).  Python-size integers: no difference overflows."""
    d = depth.astype(np.int64)
    m = d > 0
    right, down = np.zeros(d.shape, bool), np.zeros(d.shape, bool)
    right[:, :-1] = m[:, :-1] & m[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= jump_mm)
    down[:-1, :] = m[:-1, :] & m[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= jump_mm)
    return m, right, down


def roots_by_flood_fill(depth, jump_mm):
    """uint32[h, w]: the lowest pixel index of every pixel's component, NO_ROOT where nothing is measured.  Pixels are visited in index order, so
    the pixel a fill starts from is its component's root."""
    h, w = depth.shape
    m, right, down = links(depth, jump_mm)
    m, right, down = m.tolist(), right.tolist(), down.tolist()
    root = [[NO_ROOT] * w for _ in range(h)]
    for y0 in range(h):
        for x0 in range(w):
            if not m[y0][x0] or root[y0][x0] != NO_ROOT:
                continue
            r = y0 * w + x0
            root[y0][x0] = r
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                if right[y][x] and root[y][x + 1] == NO_ROOT:
                    root[y][x + 1] = r
                    stack.append((y, x + 1))
                if x > 0 and right[y][x - 1] and root[y][x - 1] == NO_ROOT:
                    root[y][x - 1] = r
                    stack.append((y, x - 1))
                if down[y][x] and root[y + 1][x] == NO_ROOT:
                    root[y + 1][x] = r
                    stack.append((y + 1, x))
                if y > 0 and down[y - 1][x] and root[y - 1][x] == NO_ROOT:
                    root[y - 1][x] = r
                    stack.append((y - 1, x))
    return np.array(root, dtype=np.uint32).reshape(h, w)


def scene_segments(depth, jump_mm=10, min_pixels=256, max_segments=64):
    """dict(segments RECORD[n_found], labels uint16[h, w], roots uint32[h, w], counts (n_found, n_qualifying, n_components)); Refused as the library refuses"""
    check_params(jump_mm, min_pixels, max_segments)
    h, w = depth.shape
    check_frame(w, h)
    roots = roots_by_flood_fill(depth, jump_mm)
    flat = roots.reshape(-1)
    measured = flat != NO_ROOT
    ids, pixels = np.unique(flat[measured], return_counts=True)
    qualifying = [(int(r), int(n)) for r, n in zip(ids, pixels) if n >= min_pixels]
    if len(qualifying) > SEGMENT_MAX_ROOTS:
        raise Refused("roots")
    qualifying.sort(key=lambda rn: (-rn[1], rn[0]))
    found = qualifying[:max_segments]
    labels = np.where(measured, SEGMENT_DROPPED, 0).astype(np.uint16)
    segs = np.zeros(len(found), RECORD)
    d = depth.reshape(-1).astype(np.int64)
    for k, (r, n) in enumerate(found):
        px = np.flatnonzero(flat == r)
        labels[px] = k + 1
        xs, ys = px % w, px // w
        segs[k] = (r, n, xs.min(), ys.min(), xs.max(), ys.max(), d[px].min(), d[px].max(), int(xs.sum()), int(ys.sum()), int(d[px].sum()), (0, 0))
    return dict(segments=segs, labels=labels.reshape(h, w), roots=roots, counts=(len(found), len(qualifying), len(ids)))


def roots_by_min_propagation(depth, jump_mm):
    """the second formulation: every measured pixel starts with its own index and takes the minimum over its linked 4-neighbours until nothing changes"""
    h, w = depth.shape
    m, right, down = links(depth, jump_mm)
    big = np.int64(2 ** 40)
    lab = np.where(m, np.arange(h * w, dtype=np.int64).reshape(h, w), big)
    while True:
        new = lab.copy()
        np.minimum(new[:, :-1], np.where(right[:, :-1], lab[:, 1:], big), out=new[:, :-1])
        np.minimum(new[:, 1:], np.where(right[:, :-1], lab[:, :-1], big), out=new[:, 1:])
        np.minimum(new[:-1, :], np.where(down[:-1, :], lab[1:, :], big), out=new[:-1, :])
        np.minimum(new[1:, :], np.where(down[:-1, :], lab[:-1, :], big), out=new[1:, :])
        # a sweep along each axis carries a minimum the whole way in one turn where the links allow it
        for x in range(1, w):
            np.minimum(new[:, x], np.where(right[:, x - 1], new[:, x - 1], big), out=new[:, x])
        for x in range(w - 2, -1, -1):
            np.minimum(new[:, x], np.where(right[:, x], new[:, x + 1], big), out=new[:, x])
        for y in range(1, h):
            np.minimum(new[y], np.where(down[y - 1], new[y - 1], big), out=new[y])
        for y in range(h - 2, -1, -1):
            np.minimum(new[y], np.where(down[y], new[y + 1], big), out=new[y])
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(m, lab, NO_ROOT).astype(np.uint32)


def segment_roi(seg, width, height, margin=0):
    x0, y0 = max(int(seg["x0"]) - margin, 0), max(int(seg["y0"]) - margin, 0)
    x1, y1 = min(int(seg["x1"]) + margin, width - 1), min(int(seg["y1"]) + margin, height - 1)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def segment_depth(labels, depth, keep):
    keep = np.atleast_1d(np.asarray(keep)).astype(np.int64)
    return np.where(np.isin(labels.astype(np.int64), keep) & (labels != 0) & (labels != SEGMENT_DROPPED), depth, 0).astype(depth.dtype)
