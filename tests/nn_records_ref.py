"""What the kd-tree searches' derived data must satisfy, stated from the caller's nodes and points alone (numpy only).

`check_records(nodes, pts, max_dist, R, camera)` holds a record set `R` (the arrays of api.debug_nn_records) to the tree and the points it
encodes; `build_records` is a plain restatement of the builders (nn_build.hip, the grid kernels of nn_search.hip) that the host tests
use to make record sets by hand.  Nothing here reads an intermediate array of the device: subtree point sets come from the nodes'
child links and the leaves' left / right, exact boxes are computed bottom-up over the points, and a dequantised value is compared with
a coordinate on the float32 values themselves (as float64, exactly).

Looseness bound (asserted where a unit of the frame is at least an ulp of the largest coordinate on that axis): a stored corner lies at
most 4 units beyond the real-number outward rounding floor((lo - origin) / unit) resp. ceil((hi - origin) / unit).  Derivation: the
float32 difference lo - origin errs by at most half an ulp of a coordinate, i.e. at most half a unit, and the division by less than
0.01 unit, so the converted value is less than one unit from the real quotient; the builders then start from floor - 1 resp. ceil + 1,
two units in all with the conversion's; the fix-up loop moves a corner further only while the dequantised float32 value -- itself at
most an ulp, i.e. a unit, off its real position -- is still on the wrong side of the coordinate: one or two more.  A larger value in a
well-conditioned case is a finding to explain, not a constant to raise.  Maxima seen: profiles/nn_records/README.md.
"""
from __future__ import annotations

import numpy as np

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
FLT_MAX = np.finfo(F32).max
K_WIDE_LEAF, K_WIDE_EMPTY = 0x80000000, 0xFFFFFFFF
K_WIDE_MAX_LEAF, K_WIDE_FIRST_MASK, K_WIDE_CHUNK = 15, 0x07FFFFFF, 1024
MAX_LOOSE_UNITS = 4


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding (a * b must be exact in float64: at most 53 significant bits between the two)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    t = p + c
    bp = t - p
    e = (p - (t - bp)) + (c - bp)                                  # TwoSum: t + e is the exact sum
    with np.errstate(over="ignore"):
        r = t.astype(F32)
    d = t - r.astype(F64)
    other = np.where(d > 0, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf)))
    with np.errstate(invalid="ignore", over="ignore"):
        tie = np.isfinite(r) & (d != 0) & (np.abs(d) * 2 == np.abs(other.astype(F64) - r.astype(F64)))
    fix = tie & (e != 0)                                           # float64 landed on a float32 midpoint, the exact sum did not
    r = np.where(fix & (e > 0), np.maximum(r, other), r)
    r = np.where(fix & (e < 0), np.minimum(r, other), r)
    return r.astype(F32)


def deq(q, qmin, qs):
    """nn_deq: qmin + (float)q * qscale, two roundings."""
    return (F32(qmin) + np.asarray(q).astype(F32) * F32(qs)).astype(F32)


def deq_fma(q, qmin, qs):
    """nn_deq_fma: fma((float)q, qscale, qmin)."""
    return fma32(np.asarray(q).astype(F32), F32(qs), F32(qmin))


# ---- the tree as the caller states it ----------------------------------------------------------------------------------------------
class Tree:
    """Links, subtree hulls, reference boxes and child sizes of a Node_kdtree array over `pts` (float32 (n, 3))."""

    def __init__(self, nodes, pts):
        self.nodes = nodes
        self.pts = pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
        n = self.n = len(nodes)
        self.c1, self.c2 = nodes["child1"].astype(np.int64), nodes["child2"].astype(np.int64)
        self.leaf = (self.c1 < 0) | (self.c2 < 0)
        self.left, self.right = nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
        self.dim = nodes["split_dim"].astype(np.int64) & 3
        order, depth = [], np.zeros(n, np.int64)
        stack = [0]
        seen = np.zeros(n, bool)
        while stack:                                                # pre-order from the root along the child links
            i = stack.pop()
            assert not seen[i], f"node {i} reached twice: not a tree"
            seen[i] = True
            order.append(i)
            if not self.leaf[i]:
                for c in (self.c2[i], self.c1[i]):
                    assert 0 <= c < n, f"node {i}: child {c} outside the array"
                    depth[c] = depth[i] + 1
                    stack.append(int(c))
        assert seen.all(), "nodes that the root does not reach"
        self.order, self.node_depth = order, depth
        self.depth = int(depth.max())
        # exact hull of every subtree, bottom-up over the points
        lo = np.full((n, 3), FLT_MAX, F32); hi = np.full((n, 3), -FLT_MAX, F32)
        for i in reversed(order):
            if self.leaf[i]:
                p = pts[self.left[i]:self.right[i]]
                if len(p):
                    lo[i], hi[i] = p.min(0), p.max(0)
            else:
                lo[i] = np.minimum(lo[self.c1[i]], lo[self.c2[i]]); hi[i] = np.maximum(hi[self.c1[i]], hi[self.c2[i]])
        self.hull_lo, self.hull_hi = lo, hi
        # the boxes the records carry: a leaf's hull, an internal node's bbox
        bb = np.asarray(nodes["bbox"], F32)
        self.box_lo = np.where(self.leaf[:, None], lo, bb[:, 0::2]).astype(F32)
        self.box_hi = np.where(self.leaf[:, None], hi, bb[:, 1::2]).astype(F32)
        # "size" of a node as its parent records it: squared diagonal of its bbox in the builder's operation order, -1 for a leaf
        d = (bb[:, 1::2] - bb[:, 0::2]).astype(F32)
        sz = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2]).astype(F32)
        self.size = np.where(self.leaf, F32(-1.0), sz).astype(F32)

    def children_follow(self):
        it = ~self.leaf
        idx = np.arange(self.n)
        return bool(np.all((self.c1[it] > idx[it]) & (self.c2[it] > idx[it])))


def frontier(t: Tree, root: int):
    """The slots of the wide node whose binary root is `root` (nn_wide_open_kernel): the root is always opened, then the slot of the
    largest size, the lowest slot on equal sizes; the first child takes its place, the second the next free slot."""
    slots = [root]
    sizes = [F32(-1.0) if t.leaf[root] else FLT_MAX]
    while len(slots) < 8:
        pick = int(np.argmax(np.array(sizes, F32)))                 # argmax: the first of the largest
        if not sizes[pick] >= 0:
            break
        node = slots[pick]
        a, b = int(t.c1[node]), int(t.c2[node])
        slots[pick], sizes[pick] = a, t.size[a]
        slots.append(b); sizes.append(t.size[b])
    return slots


def wide_topology(t: Tree):
    """(roots, slots, level): binary root and slots (binary node ids) of every wide node in level order -- wide node k's internal slots
    are numbered after everything numbered before, slot by slot -- and the wide level of each."""
    roots, slots, level = [0], [], [0]
    k = 0
    while k < len(roots):
        s = frontier(t, roots[k])
        slots.append(s)
        for b in s:
            if not t.leaf[b]:
                roots.append(b); level.append(level[k] + 1)
        k += 1
    return roots, slots, np.array(level)


def level_sizes(level):
    return np.bincount(level)


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def frames(t: Tree, max_dist):
    """info[2..7], info[16..19], info[20] of nn_frame_kernel, in float32."""
    lo, hi = t.box_lo[0], t.box_hi[0]
    qmin = lo.copy()
    qs = np.empty(3, F32)
    for a in range(3):
        sc = F32(F32(F32(hi[a] - lo[a]) / F32(65535.0)) * F32(1.000001))
        qs[a] = sc if sc > F32(1e-30) else F32(1e-30)
    margin = F32(F32(max_dist) * F32(1.01))
    if not (margin >= 0 and margin < F32(1e30)):
        margin = F32(0)
    edge = F32(max(F32(hi[0] - lo[0]), F32(hi[1] - lo[1]), F32(hi[2] - lo[2])) + F32(F32(2.0) * margin))
    wsc = F32(F32(edge / F32(65535.0)) * F32(1.000001))
    if not wsc > F32(1e-30):
        wsc = F32(1e-30)
    wmin = (lo - margin).astype(F32)
    cmax = F32(0)
    for a in range(3):
        cmax = max(cmax, abs(F32(lo[a] - margin)), abs(F32(hi[a] + margin)))
    ok = bool(F32(cmax * F32(1.1920929e-7)) <= wsc and cmax < F32(1e30))
    return qmin, qs, wmin, wsc, ok, margin


def quantise(lo, hi, qmin, qs, dq):
    """Outward 16-bit corners of boxes (k, 3) in a frame, as the builders compute them; (ql, qh, ok)."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    ql = np.zeros(lo.shape, np.int64); qh = np.zeros(lo.shape, np.int64); ok = np.ones(len(lo), bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(3):
            m, s = F32(qmin[a]), F32(qs[a])
            fl = np.floor(((lo[:, a] - m).astype(F32) / s).astype(F32)) - F32(1.0)
            l = np.where(fl > 0, np.where(fl < 65535.0, fl, 65535.0), 0.0)
            l = np.nan_to_num(l, nan=0.0).astype(np.int64)
            while True:
                bad = (l > 0) & ~(dq(l, m, s) <= lo[:, a])
                if not bad.any():
                    break
                l[bad] -= 1
            ok &= dq(l, m, s) <= lo[:, a]
            fh = np.ceil(((hi[:, a] - m).astype(F32) / s).astype(F32)) + F32(1.0)
            h = np.where(fh > 0, np.where(fh < 65535.0, fh, 65535.0), 0.0)
            h = np.nan_to_num(h, nan=0.0).astype(np.int64)
            while True:
                bad = (h < 65535) & ~(dq(h, m, s) >= hi[:, a])
                if not bad.any():
                    break
                h[bad] += 1
            ok &= dq(h, m, s) >= hi[:, a]
            ql[:, a], qh[:, a] = l, h
    return ql, qh, ok


def representable(lo, hi, qmin, qs, dq):
    """Does an outward 16-bit box exist at all?  (dequantisation is monotone: the extreme codes decide)"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    ok = np.ones(len(lo), bool)
    for a in range(3):
        ok &= (dq(np.zeros(len(lo), np.int64), qmin[a], qs[a]) <= lo[:, a]) & (dq(np.full(len(lo), 65535), qmin[a], qs[a]) >= hi[:, a])
    return ok


def unpack_wide(wide):
    """Undo nn_wide_layout_kernel: (n, 32) words -> boxes (n, 8, 6) {lo.xyz, hi.xyz} and references (n, 8)."""
    w = np.ascontiguousarray(wide, U32).reshape(-1, 2, 16)
    pairs = w[:, :, :12].reshape(-1, 2, 2, 6)                        # [node, half, pair, field]: first slot | second slot << 16
    box = np.stack([pairs & 0xFFFF, pairs >> 16], axis=3)            # [node, half, pair, which, field]
    return box.reshape(-1, 8, 6).astype(np.int64), w[:, :, 12:16].reshape(-1, 8).copy()


def pack_wide(box, ref):
    box = np.asarray(box, U32).reshape(-1, 2, 2, 2, 6)
    w = np.zeros((len(box), 2, 16), U32)
    w[:, :, :12] = (box[:, :, :, 0, :] | (box[:, :, :, 1, :] << 16)).reshape(-1, 2, 12)
    w[:, :, 12:16] = np.asarray(ref, U32).reshape(-1, 2, 4)
    return w.reshape(-1, 32)


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
def grid_cells(w, h):
    total = w * h
    for _ in range(3):
        w, h = (w + 3) // 4, (h + 3) // 4
        total += w * h
    return total


def grid_pixels(pts, cam):
    """grid_pixel in float32: (px, py, valid) -- valid = z > 0, a finite projection, inside the image."""
    w, h, fx, fy, cx, cy = cam
    p = np.ascontiguousarray(pts, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (((p[:, 0] / p[:, 2]).astype(F32) * F32(fx)).astype(F32) + F32(cx)).astype(F32) + F32(0.5)
        v = (((p[:, 1] / p[:, 2]).astype(F32) * F32(fy)).astype(F32) + F32(cy)).astype(F32) + F32(0.5)
        fin = (u > F32(-1e6)) & (u < F32(1e6)) & (v > F32(-1e6)) & (v < F32(1e6))
        px = np.where(fin, np.floor(u), -1).astype(np.int64); py = np.where(fin, np.floor(v), -1).astype(np.int64)
    ok = (p[:, 2] > 0) & fin & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    return px, py, ok


def build_grid(pts, cam):
    """(usable, cell_idx (h, w) int32, grid (cells, 4) float32); the arrays mean something only when usable."""
    w, h = int(cam[0]), int(cam[1])
    px, py, ok = grid_pixels(pts, cam)
    cell = py * w + px
    usable = bool(ok.all() and len(np.unique(cell)) == len(cell))
    idx = np.full(w * h, -1, I32)
    if usable:
        idx[cell] = np.arange(len(cell), dtype=I32)
    levels = [np.zeros((h, w, 4), F32)]
    g = levels[0].reshape(-1, 4)
    g[:, :3] = F32(1e30)
    g[:, 3] = np.array([-1], I32).view(F32)[0]
    occ = idx >= 0
    g[occ, :3] = np.ascontiguousarray(pts, F32)[idx[occ]]
    g[occ, 3] = idx[occ].view(F32)
    fw, fh = w, h
    for _ in range(3):
        cw, ch = (fw + 3) // 4, (fh + 3) // 4
        fine = levels[-1]
        pad = np.zeros((ch * 4, cw * 4, 4), F32)
        pad[:, :, :3] = F32(1e30); pad[:, :, 3] = np.array([-1], I32).view(F32)[0]
        pad[:fh, :fw] = fine
        coarse = np.zeros((ch, cw, 4), F32)
        coarse[:, :, :3] = F32(1e30); coarse[:, :, 3] = np.array([-1], I32).view(F32)[0]
        best = np.full((ch, cw), 1 << 30, np.int64)
        for dy in range(4):                                          # scan order: a strictly nearer occupied child replaces
            for dx in range(4):
                v = pad[dy::4, dx::4]
                dist = (2 * dx - 3) ** 2 + (2 * dy - 3) ** 2
                take = (np.ascontiguousarray(v[:, :, 3]).view(I32) >= 0) & (dist < best)
                coarse[take] = v[take]; best[take] = dist
        levels.append(coarse)
        fw, fh = cw, ch
    return usable, idx.reshape(h, w), np.concatenate([l.reshape(-1, 4) for l in levels])


# ---- a plain restatement of the builders (hand-made record sets of the host tests) -------------------------------------------------
def build_records(nodes, pts, max_dist, camera=None):
    """A record set as the builders would make it (the arrays of api.debug_nn_records, plus "grid_usable" when a grid is built)."""
    t = Tree(nodes, pts)
    n = t.n
    qmin, qs, wmin, wsc, wide_ok, _ = frames(t, max_dist)
    base = build_topology(t)
    topo, bmin, bmax, rec64 = base["topo"], base["bmin"], base["bmax"], base["rec64"]
    rec32 = np.zeros((n, 8), U32)
    rec32[:, 0] = topo[:, 0].view(U32)
    rec32[:, 1] = np.where(t.leaf, t.right | (3 << 30), t.c1 | (t.dim << 30)).astype(U32)
    it = np.flatnonzero(~t.leaf)
    ok32 = compact_ok(t, qmin, qs)
    q = np.zeros((n, 12), np.int64)
    good = it[ok32[it]]
    for c, ch in enumerate((t.c1, t.c2)):
        ql, qh, _ = quantise(t.box_lo[ch[good]], t.box_hi[ch[good]], qmin, qs, deq)
        q[good, 6 * c:6 * c + 3], q[good, 6 * c + 3:6 * c + 6] = ql, qh
    bad = it[~ok32[it]]                                              # (a node that does not fit carries node 0's box twice)
    if len(bad):
        ql, qh, _ = quantise(t.box_lo[:1], t.box_hi[:1], qmin, qs, deq)
        q[bad] = np.concatenate([ql, qh, ql, qh], 1)
    rec32[:, 2:] = (q[:, 0::2] | (q[:, 1::2] << 16)).astype(U32)
    info = np.zeros(24, U32)
    info[0] = t.depth
    info[1] = 1 if ok32[it].all() else 0
    info[2:5], info[5:8] = bits(qmin), bits(qs)
    info[16:19], info[19], info[20] = bits(wmin), bits(np.array([wsc], F32))[0], int(wide_ok)
    R = {"topo": topo, "bmin": bmin, "bmax": bmax, "rec64": rec64, "rec32": rec32, "desc": rec32[:, :2].copy(),
         "pts": np.concatenate([t.pts, np.zeros((len(t.pts), 1), F32)], 1), "info": info, "wide": np.zeros((0, 32), U32), "cell_idx": None, "grid": None}
    if expect_wide(t, info):
        roots, slots, _ = wide_topology(t)
        number = {b: k for k, b in enumerate(roots)}
        box = np.zeros((len(roots), 8, 6), np.int64); ref = np.full((len(roots), 8), K_WIDE_EMPTY, np.int64)
        flat = np.array([b for s in slots for b in s])
        ql, qh, okq = quantise(t.box_lo[flat], t.box_hi[flat], wmin, [wsc] * 3, deq_fma)
        assert okq.all()
        at = 0
        for k, s in enumerate(slots):
            for c, b in enumerate(s):
                box[k, c] = np.concatenate([ql[at], qh[at]]); at += 1
                ref[k, c] = (K_WIDE_LEAF | ((t.right[b] - t.left[b]) << 27) | t.left[b]) if t.leaf[b] else number[b]
        R["wide"] = pack_wide(box, ref)
        info[8], info[9] = 1, len(roots)
    else:
        info[9] = 1
    if camera is not None and info[1] == 1:
        usable, R["cell_idx"], R["grid"] = build_grid(t.pts, camera)
        R["grid_usable"] = usable
    return R


def compact_ok(t: Tree, qmin, qs):
    """Per node: may it be a compact record?  child2 == child1 + 1, dim < 3, left_max <= split <= right_min, representable boxes."""
    ok = np.ones(t.n, bool)
    it = np.flatnonzero(~t.leaf)
    c1, c2, dim = t.c1[it], t.c2[it], t.dim[it]
    good = (c2 == c1 + 1) & (c1 < (1 << 30)) & (dim < 3) & (c2 < t.n)
    d = np.minimum(dim, 2)
    lmax, rmin = t.box_hi[c1, d], t.box_lo[np.minimum(c2, t.n - 1), d]
    split = np.asarray(t.nodes["split_v"], F32)[it]
    good &= (lmax <= split) & (split <= rmin)
    for ch in (c1, np.minimum(c2, t.n - 1)):
        good &= representable(t.box_lo[ch], t.box_hi[ch], qmin, qs, deq)
    ok[it] = good
    return ok


def expect_wide(t: Tree, info):
    """info[8] == 1 exactly when the compact records and the wide frame are usable, leaves hold at most 15 points and children follow
    their parents.  (A leaf without points has no leaf reference; such trees are outside this statement and count as not expressible.)"""
    cnt = (t.right - t.left)[t.leaf]
    return bool(info[1] == 1 and info[20] == 1 and cnt.max() <= K_WIDE_MAX_LEAF and cnt.min() >= 1 and t.children_follow())


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def real_units(x, origin, unit):
    """(x - origin) / unit in real numbers (float64 of float32 values: the quotient's error is far below the distance of any of these
    values to an integer that matters for a bound of whole units)."""
    return (np.asarray(x, F64) - F64(origin)) / F64(unit)


def looseness(ql, qh, lo, hi, origin, unit):
    """Units a stored corner lies beyond the real-number outward rounding, per box and axis: (lo side, hi side)."""
    out = []
    for a in range(3):
        il = np.clip(np.floor(real_units(lo[:, a], origin[a], unit[a])), 0, 65535)
        ih = np.clip(np.ceil(real_units(hi[:, a], origin[a], unit[a])), 0, 65535)
        out.append((il - ql[:, a], qh[:, a] - ih))
    return out


def well_conditioned(unit, cmax):
    """Is a unit of the frame at least an ulp of the largest coordinate on that axis?"""
    return bool(F32(unit) >= np.spacing(F32(cmax)))


def check_records(nodes, pts, max_dist, R, camera=None, n_queries=48, seed=0):
    """Every statement of the module docstring, asserted.  Returns a report: counts and the looseness maxima."""
    t = Tree(nodes, pts)
    n = t.n
    info = np.asarray(R["info"], U32)
    rep = {"n_nodes": n, "n_points": len(t.pts), "depth": t.depth}
    # -- topology and boxes
    want = build_topology(t)
    assert np.array_equal(np.asarray(R["topo"], I32), want["topo"]), "topo does not restate the links"
    for k in ("bmin", "bmax"):
        got = bits(R[k]).reshape(n, 4)
        assert np.array_equal(got[:, :3], bits(want[k][:, :3]).reshape(n, 3)), f"{k}: a leaf's box is the hull of its points, an internal node's its bbox"
        assert np.array_equal(got[:, 3], bits(want[k][:, 3])), f"{k}.w: the children's squared diagonals (float32, the builder's order), -1 for a leaf"
    assert np.array_equal(bits(R["pts"]).reshape(-1, 4), bits(np.concatenate([t.pts, np.zeros((len(t.pts), 1), F32)], 1)).reshape(-1, 4)), "pts"
    # -- 64-byte records
    assert np.array_equal(bits(R["rec64"]).reshape(n, 16), bits(want["rec64"]).reshape(n, 16)), "rec64: links, and the children's boxes bit for bit"
    assert info[0] == t.depth, ("info[0] is the depth of the tree", info[0], t.depth)
    # -- compact records
    qmin, qs, wmin, wsc, wide_ok, margin = frames(t, max_dist)
    assert np.array_equal(info[2:5], bits(qmin)) and np.array_equal(info[5:8], bits(qs)), "the compact frame"
    assert np.array_equal(info[16:19], bits(wmin)) and info[19] == bits(np.array([wsc], F32))[0], "the wide frame"
    assert info[20] == int(wide_ok), ("info[20]", info[20], wide_ok)
    rec32 = np.asarray(R["rec32"], U32)
    assert np.array_equal(np.asarray(R["desc"], U32), rec32[:, :2]), "desc is the first two words of rec32"
    assert np.array_equal(rec32[:, 0], want["topo"][:, 0].view(U32)), "rec32 word 0"
    assert np.array_equal(rec32[:, 1], np.where(t.leaf, t.right | (3 << 30), t.c1 | (t.dim << 30)).astype(U32)), "rec32 word 1"
    it = np.flatnonzero(~t.leaf)
    ok32 = compact_ok(t, qmin, qs)
    assert info[1] == (1 if ok32[it].all() else 0), ("info[1]", info[1], int(ok32[it].all()))
    root_abs = np.maximum(np.abs(t.box_lo[0]), np.abs(t.box_hi[0]))
    rep["compact_loose"], rep["compact_loose_asserted"] = 0, [well_conditioned(qs[a], root_abs[a]) for a in range(3)]
    if info[1] == 1 and len(it):
        q = np.ascontiguousarray(rec32[it, 2:]).view(np.uint16).reshape(len(it), 12).astype(np.int64)
        for c, ch in enumerate((t.c1[it], t.c2[it])):
            ql, qh = q[:, 6 * c:6 * c + 3], q[:, 6 * c + 3:6 * c + 6]
            for a in range(3):
                assert np.all(deq(ql[:, a], qmin[a], qs[a]).astype(F64) <= t.hull_lo[ch, a].astype(F64)), f"compact box of child {c + 1}: lower corner inside the hull (axis {a})"
                assert np.all(deq(qh[:, a], qmin[a], qs[a]).astype(F64) >= t.hull_hi[ch, a].astype(F64)), f"compact box of child {c + 1}: upper corner inside the hull (axis {a})"
            for a, (l, h) in enumerate(looseness(ql, qh, t.box_lo[ch], t.box_hi[ch], qmin, qs)):
                m = int(max(l.max(), h.max()))
                if rep["compact_loose_asserted"][a]:
                    rep["compact_loose"] = max(rep["compact_loose"], m)
                    assert m <= MAX_LOOSE_UNITS, f"compact box of child {c + 1}, axis {a}: {m} units beyond the outward rounding"
    # -- wide records
    assert info[8] == (1 if expect_wide(t, info) else 0), ("info[8]", info[8], expect_wide(t, info))
    rep["wide_usable"], rep["n_wide"], rep["wide_levels"], rep["continued"] = int(info[8]), 0, 0, False
    rep["wide_loose"] = 0
    if info[8] == 1:
        roots, slots, level = wide_topology(t)
        rep["n_wide"], rep["wide_levels"], rep["continued"] = len(roots), int(level.max()) + 1, bool(level.max() + 1 > 8)
        rep["level_sizes"] = level_sizes(level).tolist()
        assert info[9] == len(roots) == len(R["wide"]), ("info[9] wide nodes", info[9], len(roots), len(R["wide"]))
        box, ref = unpack_wide(R["wide"])
        check_wide(t, box, ref, roots, slots, wmin, wsc, margin, rep)
        check_walk_bound(t, box, ref, wmin, wsc, max_dist, margin, n_queries, seed)
    # -- grid
    if camera is not None and R.get("grid") is not None:
        usable, idx, grid = build_grid(t.pts, camera)
        assert bool(R["grid_usable"]) == usable, ("grid usable", R["grid_usable"], usable)
        assert len(R["grid"]) == grid_cells(int(camera[0]), int(camera[1])), "nn_grid_cells"
        rep["grid_usable"] = usable
        if usable:
            assert np.array_equal(np.asarray(R["cell_idx"], I32), idx), "cell -> the point that projects into it"
            assert np.array_equal(bits(R["grid"]).reshape(-1, 4), bits(grid).reshape(-1, 4)), "grid: the point's own xyz and index, empty cells (1e30, 1e30, 1e30, -1), coarser levels"
    return rep


def build_topology(t: Tree):
    nodes = t.nodes
    n = t.n
    pw = (((nodes["parent"].astype(np.int64) + 1) & 0x3FFFFFFF) | (t.dim << 30)).astype(U32).view(I32)
    topo = np.zeros((n, 4), I32)
    topo[:, 0] = np.where(t.leaf, t.left, bits(nodes["split_v"]).view(I32))
    topo[:, 1] = np.where(t.leaf, t.right, t.c1); topo[:, 2] = np.where(t.leaf, -1, t.c2); topo[:, 3] = pw
    c1, c2 = np.where(t.leaf, 0, t.c1), np.where(t.leaf, 0, t.c2)
    bmin = np.zeros((n, 4), F32); bmax = np.zeros((n, 4), F32)
    bmin[:, :3], bmax[:, :3] = t.box_lo, t.box_hi
    bmin[:, 3] = np.where(t.leaf, F32(0), t.size[c1]); bmax[:, 3] = np.where(t.leaf, F32(0), t.size[c2])
    rec64 = np.zeros((n, 16), F32)
    rec64[:, :3] = topo[:, :3].view(F32)
    rec64[:, 3] = np.where(t.leaf, F32(0), np.ascontiguousarray(t.dim.astype(I32)).view(F32))
    kids = np.concatenate([t.box_lo[c1], t.box_hi[c1], t.box_lo[c2], t.box_hi[c2]], 1)
    rec64[:, 4:] = np.where(t.leaf[:, None], F32(0), kids)
    return {"topo": topo, "bmin": bmin, "bmax": bmax, "rec64": rec64}


def check_wide(t: Tree, box, ref, roots, slots, wmin, wsc, margin, rep):
    nw = len(roots)
    number = {b: k for k, b in enumerate(roots)}
    want = np.full((nw, 8), K_WIDE_EMPTY, np.int64)
    for k, s in enumerate(slots):
        for c, b in enumerate(s):
            want[k, c] = (K_WIDE_LEAF | ((t.right[b] - t.left[b]) << 27) | t.left[b]) if t.leaf[b] else number[b]
    # from wide node 0, every point index exactly once (the records' own references, not the restatement's)
    seen_pt = np.zeros(len(t.pts), np.int64); seen_w = np.zeros(nw, np.int64)
    lo = np.full((nw, 8, 3), FLT_MAX, F32); hi = np.full((nw, 8, 3), -FLT_MAX, F32)
    todo = [0]; seen_w[0] = 1
    while todo:
        k = todo.pop()
        for c in range(8):
            r = int(ref[k, c])
            if r == K_WIDE_EMPTY:
                continue
            if r & K_WIDE_LEAF:
                first, cnt = r & K_WIDE_FIRST_MASK, (r >> 27) & 15
                assert cnt >= 1 and first + cnt <= len(t.pts), f"wide node {k} slot {c}: leaf reference outside the points"
                seen_pt[first:first + cnt] += 1
            else:
                assert r < nw, f"wide node {k} slot {c}: reference {r} outside the {nw} wide nodes"
                seen_w[r] += 1
                if seen_w[r] == 1:
                    todo.append(r)
    assert np.all(seen_pt >= 1), f"points that no leaf of the wide tree holds: {np.flatnonzero(seen_pt == 0)[:8]}"
    assert np.all(seen_pt == 1), f"points reached more than once: {np.flatnonzero(seen_pt > 1)[:8]}"
    assert np.all(seen_w == 1), "every wide node hangs under exactly one slot"
    assert np.array_equal(ref.astype(np.int64), want), "the same references in the same slots"
    # hull of what hangs under every slot, from the records' references, bottom-up (children are numbered after their parents)
    node_lo = np.full((nw, 3), FLT_MAX, F32); node_hi = np.full((nw, 3), -FLT_MAX, F32)
    for k in range(nw - 1, -1, -1):
        for c in range(8):
            r = int(ref[k, c])
            if r == K_WIDE_EMPTY:
                continue
            if r & K_WIDE_LEAF:
                p = t.pts[(r & K_WIDE_FIRST_MASK):(r & K_WIDE_FIRST_MASK) + ((r >> 27) & 15)]
                lo[k, c], hi[k, c] = p.min(0), p.max(0)
            else:
                assert r > k
                lo[k, c], hi[k, c] = node_lo[r], node_hi[r]
        node_lo[k], node_hi[k] = lo[k].min(0), hi[k].max(0)
    used = ref != K_WIDE_EMPTY
    assert np.all(box[~used] == 0), "empty slots carry zero boxes"
    b, l, h = box[used], lo[used], hi[used]
    for a in range(3):
        assert np.all(deq_fma(b[:, a], wmin[a], wsc).astype(F64) <= l[:, a].astype(F64)), f"wide box: lower corner inside the hull (axis {a})"
        assert np.all(deq_fma(b[:, 3 + a], wmin[a], wsc).astype(F64) >= h[:, a].astype(F64)), f"wide box: upper corner inside the hull (axis {a})"
    # looseness against the box the slot's binary node carries
    flat = np.array([x for s in slots for x in s])
    order = np.array([(k, c) for k, s in enumerate(slots) for c in range(len(s))])
    sb = box[order[:, 0], order[:, 1]]
    cabs = np.maximum(np.abs(wmin), np.abs((t.box_hi[0] + margin).astype(F32)))
    for a, (dl, dh) in enumerate(looseness(sb[:, :3], sb[:, 3:], t.box_lo[flat], t.box_hi[flat], wmin, [wsc] * 3)):
        if well_conditioned(wsc, cabs[a]):
            m = int(max(dl.max(), dh.max()))
            rep["wide_loose"] = max(rep["wide_loose"], m)
            assert m <= MAX_LOOSE_UNITS, f"wide box, axis {a}: {m} units beyond the outward rounding"


def sq_dist(q, pts):
    dx = q[:, None, 0] - pts[None, :, 0]; dy = q[:, None, 1] - pts[None, :, 1]; dz = q[:, None, 2] - pts[None, :, 2]
    return ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)


def sample_queries(t: Tree, margin, n, seed):
    """Inside the root box, outside it but within the margin, and beyond the margin on each side."""
    rng = np.random.default_rng(seed)
    lo, hi = t.box_lo[0].astype(F64), t.box_hi[0].astype(F64)
    m = float(margin)
    q = [rng.uniform(lo, hi, size=(n, 3)), t.pts[rng.integers(0, len(t.pts), n)].astype(F64) + rng.normal(size=(n, 3)) * 0.3 * m]
    for a in range(3):
        for side in (0, 1):
            for dist in (rng.uniform(0, m, n // 4 + 1), rng.uniform(m, 3 * m + 1e-6, n // 4 + 1)):
                p = rng.uniform(lo, hi, size=(len(dist), 3))
                p[:, a] = (lo[a] - dist) if side == 0 else (hi[a] + dist)
                q.append(p)
    return np.ascontiguousarray(np.concatenate(q).astype(F32))


def walk_lower_bounds(box, q, wmin, wsc):
    """nn_tree_wide_kernel's integer bound of every (query, wide node, slot) in squared units, low six bits cleared as the queues carry
    it, and the factor from squared metres to squared units."""
    w_inv = F32(F32(1.0) / F32(wsc))
    to_units2 = F32(F32(w_inv * w_inv) * F32(1.000001))
    u = np.empty(q.shape, np.int64)
    for a in range(3):
        v = fma32((q[:, a] - F32(wmin[a])).astype(F32), w_inv, F32(-1.0625))
        u[:, a] = np.minimum(np.maximum(np.nan_to_num(v, nan=0.0), F32(0.0)), F32(65532.0)).astype(np.int64)      # truncation, as the cast
    qd, qu = u[:, None, None, :], u[:, None, None, :] + 3
    d = np.maximum(np.maximum(box[None, :, :, :3] - qu, 0), np.maximum(qd - box[None, :, :, 3:], 0)).astype(F64)   # saturating differences
    # fma(az, az, fma(ay, ay, ax * ax)): whole numbers below 2^16, so every product and sum is exact in float64 and each step rounds once
    lb = (d[..., 0] * d[..., 0]).astype(F32)
    lb = (d[..., 1] * d[..., 1] + lb.astype(F64)).astype(F32)
    lb = (d[..., 2] * d[..., 2] + lb.astype(F64)).astype(F32)
    return (bits(lb).reshape(lb.shape) & U32(0xFFFFFFC0)).view(F32), to_units2


def check_walk_bound(t: Tree, box, ref, wmin, wsc, max_dist, margin, n_queries, seed, raise_on_fail=True):
    """For every slot and query: if the nearest point under the slot (float32 dist_sq) is within max_dist^2, the walk's bound of the
    slot's box does not exceed fma(that distance, w_to_units2, 1) -- so the walk cannot skip it.  Returns the number of violations."""
    q = sample_queries(t, margin, n_queries, seed)
    nw = len(ref)
    D = sq_dist(q, t.pts)
    dmin = np.full((len(q), nw, 8), np.inf, F32)
    node_min = np.full((len(q), nw), np.inf, F32)
    for k in range(nw - 1, -1, -1):
        for c in range(8):
            r = int(ref[k, c])
            if r == K_WIDE_EMPTY:
                continue
            if r & K_WIDE_LEAF:
                first = r & K_WIDE_FIRST_MASK
                dmin[:, k, c] = D[:, first:first + ((r >> 27) & 15)].min(1)
            else:
                dmin[:, k, c] = node_min[:, r]
        node_min[:, k] = dmin[:, k].min(1)
    bad = 0
    accept = F32(F32(max_dist) * F32(max_dist))
    step = max(1, (1 << 22) // max(1, nw * 8))
    for a in range(0, len(q), step):
        lb, to_units2 = walk_lower_bounds(box, q[a:a + step], wmin, wsc)
        dm = dmin[a:a + step]
        live = np.isfinite(dm) & (dm <= accept)
        bound = fma32(np.where(live, dm, F32(0)), to_units2, F32(1.0))
        viol = live & ~(lb <= bound)
        bad += int(viol.sum())
        if raise_on_fail and viol.any():
            i, k, c = np.argwhere(viol)[0]
            raise AssertionError(f"the walk would skip wide node {k} slot {c} for query {q[a + i]}: bound {lb[i, k, c]} > {bound[i, k, c]} squared units, "
                                 f"nearest point under it at {dm[i, k, c]} m^2")
    return bad


# ---- case generators ---------------------------------------------------------------------------------------------------------------
def comb_tree(spine=16, seed=5):
    """A valid caller-built tree (children pairwise and after their parents, split inside the gap, bbox = hull) of a few hundred nodes
    whose wide form is deep: at every spine node a small deep branch (the rest of the spine, 8 % of the extent) sits beside a wide
    shallow one (eight single-point leaves under seven internal nodes).  The six openings a wide node has left after its root all go
    into the wide branch, so every wide level advances the spine by ONE binary level: `spine` + 1 wide levels at binary depth
    `spine` + 3.  The shrink factor keeps every box diagonal's square a normal float32 (no size underflows, so no ties among sizes).
    Returns (nodes, pts, nrm); split along x."""
    from pose_refine_amd._lib import KDNODE
    rng = np.random.default_rng(seed)
    pts, nodes = [], []

    def new_node(parent):
        nodes.append({"parent": parent, "child1": -1, "child2": -1, "split_v": 0.0, "bbox": None, "split_dim": 0, "left": 0, "right": 0})
        return len(nodes) - 1

    # points in the order of a depth-first walk (left = smaller x first): the spine's tail first, then the branches from the deepest up
    E = [0.2 * 0.08 ** k for k in range(spine)]
    tail = np.array([[0.02 * E[-1], 0.0, 0.3], [0.04 * E[-1], 0.001 * E[-1], 0.3]])
    chunks = [tail]
    for k in range(spine - 1, -1, -1):
        x = E[k] * (0.3 + 0.1 * np.arange(8))
        chunks.append(np.stack([x, rng.uniform(-0.01, 0.01, 8) * E[k], 0.3 + rng.uniform(-0.01, 0.01, 8) * E[k]], 1))
    pts = np.ascontiguousarray(np.concatenate(chunks).astype(F32))
    start = {k: 2 + 8 * (spine - 1 - k) for k in range(spine)}       # first point of branch k

    def fill(i, left, right):
        p = pts[left:right]
        nodes[i]["left"], nodes[i]["right"] = left, right
        nodes[i]["bbox"] = [p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max(), p[:, 2].min(), p[:, 2].max()]

    def split(i, left, mid, right):
        a = new_node(i); b = new_node(i)                             # pairwise, after the parent
        nodes[i]["child1"], nodes[i]["child2"] = a, b
        nodes[i]["split_v"] = float((F64(pts[mid - 1, 0]) + F64(pts[mid, 0])) / 2)
        return a, b

    def balanced(i, left, right):
        fill(i, left, right)
        if right - left == 1:
            return
        mid = (left + right) // 2
        a, b = split(i, left, mid, right)
        balanced(a, left, mid); balanced(b, mid, right)

    work = [(new_node(-1), 0)]
    pending = []
    while work:                                                      # the spine first (breadth of two per level), the branches' insides after
        i, k = work.pop()
        if k == spine:
            fill(i, 0, 2)
            continue
        fill(i, 0, start[k] + 8)
        a, b = split(i, 0, start[k], start[k] + 8)
        pending.append((b, start[k], start[k] + 8))
        work.append((a, k + 1))
    for b, l, r in pending:
        balanced(b, l, r)
    out = np.zeros(len(nodes), KDNODE)
    for i, nd in enumerate(nodes):
        for f in ("parent", "child1", "child2", "split_dim", "left", "right"):
            out[f][i] = nd[f]
        out["split_v"][i] = F32(nd["split_v"]); out["bbox"][i] = np.array(nd["bbox"], F32)
    nrm = rng.normal(size=pts.shape).astype(F32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return out, pts, np.ascontiguousarray(nrm.astype(F32))


def lattice_points(n=700, step=0.1, seed=9):
    """Points on a `step` grid (exact duplicates, zero-extent boxes, equal sizes)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.integers(-3, 4, size=(n, 3)) * step).astype(F32) + np.array([0, 0, 1], F32))


def random_points(n, seed, half=0.15):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-half, half, size=(n, 3)).astype(F32))


def host_tree(pts, max_leaf, seed=1):
    """(nodes, pts, nrm) of the library's host build (reorders copies of the arrays in place; needs no device)."""
    import ctypes as C
    from pose_refine_amd import _lib
    pts = np.array(pts, F32, order="C", copy=True)
    nrm = np.random.default_rng(seed).normal(size=pts.shape).astype(F32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.ascontiguousarray(nrm.astype(F32))
    nodes = np.zeros(2 * len(pts) + 1, _lib.KDNODE); cnt = C.c_uint32()
    _lib.check(_lib.load().pr_kdtree_build(pts.ctypes.data, nrm.ctypes.data, len(pts), max_leaf, nodes.ctypes.data, len(nodes), C.byref(cnt)))
    return np.ascontiguousarray(nodes[:cnt.value]), pts, nrm
