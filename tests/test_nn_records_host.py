"""The checker of the kd-tree searches' derived data (nn_records_ref.py) on hand-made record sets, no device: it accepts what a plain
restatement of the builders makes, REJECTS each planted violation, and the case generators of the GPU file yield what they claim."""
import ctypes as C

import numpy as np
import pytest

import nn_records_ref as N
import nn_ref
from pose_refine_amd import _lib, api

CAM = (23, 17, 30.0, 31.0, 11.25, 8.5)                              # w, h, fx, fy, cx, cy


def depth_like_points(cam=CAM, seed=3, holes=0.2):
    """One point per pixel of a small image (some pixels empty), at the pixel's centre: a scene whose grid is usable."""
    w, h, fx, fy, cx, cy = cam
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    keep = rng.random((h, w)) > holes
    z = (0.4 + 0.05 * np.sin(u / 3.0) + 0.03 * rng.random((h, w)))[keep]
    return np.ascontiguousarray(np.stack([(u[keep] - cx) / fx * z, (v[keep] - cy) / fy * z, z], 1).astype(np.float32))


@pytest.fixture(scope="module")
def small():
    nodes, pts, _ = N.host_tree(depth_like_points(), 3)
    return nodes, pts, N.build_records(nodes, pts, 0.05, CAM)


def tighten(nodes, pts, R, max_dist):
    """The same records with every box corner at the LAST code that still contains the box (looseness 0): moving any of them one unit
    inwards must then be noticed."""
    t = N.Tree(nodes, pts)
    qmin, qs, wmin, wsc, _, _ = N.frames(t, max_dist)
    R = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.items()}

    def tight(lo, hi, origin, unit, dq):
        ql, qh, _ = N.quantise(lo, hi, origin, unit, dq)
        for a in range(3):
            while True:
                m = (ql[:, a] < 65535) & (dq(ql[:, a] + 1, origin[a], unit[a]) <= lo[:, a])
                if not m.any():
                    break
                ql[m, a] += 1
            while True:
                m = (qh[:, a] > 0) & (dq(qh[:, a] - 1, origin[a], unit[a]) >= hi[:, a])
                if not m.any():
                    break
                qh[m, a] -= 1
        return ql, qh

    it = np.flatnonzero(~t.leaf)
    q = np.zeros((len(it), 12), np.int64)
    for c, ch in enumerate((t.c1[it], t.c2[it])):
        q[:, 6 * c:6 * c + 3], q[:, 6 * c + 3:6 * c + 6] = tight(t.box_lo[ch], t.box_hi[ch], qmin, qs, N.deq)
    R["rec32"][it, 2:] = (q[:, 0::2] | (q[:, 1::2] << 16)).astype(np.uint32)
    box, ref = N.unpack_wide(R["wide"])
    _, slots, _ = N.wide_topology(t)
    for k, s in enumerate(slots):
        ql, qh = tight(t.box_lo[s], t.box_hi[s], wmin, [wsc] * 3, N.deq_fma)
        box[k, :len(s), :3], box[k, :len(s), 3:] = ql, qh
    R["wide"] = N.pack_wide(box, ref)
    return R


def test_hand_made_record_sets_pass(small):
    nodes, pts, R = small
    rep = N.check_records(nodes, pts, 0.05, R, CAM)
    assert rep["wide_usable"] == 1 and rep["grid_usable"] and rep["n_wide"] > 8
    assert 1 <= rep["compact_loose"] <= 2 and 1 <= rep["wide_loose"] <= 2          # floor - 1 / ceil + 1, and at most one fix-up step
    rep = N.check_records(nodes, pts, 0.05, tighten(nodes, pts, R, 0.05), CAM)
    assert rep["compact_loose"] == 0 and rep["wide_loose"] == 0
    # one leaf (the root of its wide node is not opened), a lattice full of ties, leaves too large for a leaf reference
    for p, max_leaf, wide in ((N.random_points(1, 1), 15, 1), (N.random_points(11, 2), 15, 1), (N.lattice_points(300), 1, 1), (N.random_points(400, 3), 16, 0)):
        nd, p, _ = N.host_tree(p, max_leaf)
        assert N.check_records(nd, p, 0.1, N.build_records(nd, p, 0.1))["wide_usable"] == wide


def planted(R, **changes):
    out = dict(R)
    out.update(changes)
    return out


def test_checker_rejects_a_corner_moved_inwards_by_one_unit(small):
    nodes, pts, R = small
    T = tighten(nodes, pts, R, 0.05)
    t = N.Tree(nodes, pts)
    it = np.flatnonzero(~t.leaf)
    for word, shift in ((2, 0), (3, 16), (5, 0), (7, 16)):           # child1 lo.x, child1 hi.x, child2 lo.x, child2 hi.z
        rec32 = T["rec32"].copy()
        i = it[len(it) // 2]
        step = 1 if (word, shift) in ((2, 0), (5, 0)) else -1
        rec32[i, word] = np.uint32(int(rec32[i, word]) + (step << shift))
        with pytest.raises(AssertionError, match="compact box"):
            N.check_records(nodes, pts, 0.05, planted(T, rec32=rec32, desc=rec32[:, :2].copy()), CAM)
    box, ref = N.unpack_wide(T["wide"])
    for k, c, f, step in ((0, 0, 0, 1), (len(box) // 2, 1, 4, -1), (len(box) - 1, 0, 2, 1)):
        b = box.copy()
        b[k, c, f] += step
        with pytest.raises(AssertionError, match="wide box"):
            N.check_records(nodes, pts, 0.05, planted(T, wide=N.pack_wide(b, ref)), CAM)


def test_checker_rejects_a_lost_a_doubled_and_a_swapped_slot(small):
    nodes, pts, R = small
    box, ref = N.unpack_wide(R["wide"])
    leaf = (ref != N.K_WIDE_EMPTY) & ((ref & N.K_WIDE_LEAF) != 0)
    k, c = np.argwhere(leaf)[len(np.argwhere(leaf)) // 2]
    b, r = box.copy(), ref.copy()
    r[k, c] = N.K_WIDE_EMPTY; b[k, c] = 0
    with pytest.raises(AssertionError, match="no leaf of the wide tree holds"):
        N.check_records(nodes, pts, 0.05, planted(R, wide=N.pack_wide(b, r)), CAM)
    ke, ce = np.argwhere(ref == N.K_WIDE_EMPTY)[0]                   # a free slot takes a second copy of the leaf
    b, r = box.copy(), ref.copy()
    r[ke, ce] = ref[k, c]; b[ke, ce] = box[k, c]
    with pytest.raises(AssertionError, match="more than once"):
        N.check_records(nodes, pts, 0.05, planted(R, wide=N.pack_wide(b, r)), CAM)
    b, r = box.copy(), ref.copy()
    r[0, [1, 2]] = r[0, [2, 1]]; b[0, [1, 2]] = b[0, [2, 1]]
    with pytest.raises(AssertionError, match="same references in the same slots"):
        N.check_records(nodes, pts, 0.05, planted(R, wide=N.pack_wide(b, r)), CAM)


def test_checker_rejects_a_desc_word_and_a_grid_cell(small):
    nodes, pts, R = small
    desc = R["desc"].copy()
    desc[len(desc) // 3, 1] ^= 1
    with pytest.raises(AssertionError, match="desc is the first two words"):
        N.check_records(nodes, pts, 0.05, planted(R, desc=desc), CAM)
    idx = R["cell_idx"].copy()
    occ = np.argwhere(idx >= 0)
    (y0, x0), (y1, x1) = occ[3], occ[4]
    idx[y0, x0], idx[y1, x1] = idx[y1, x1], idx[y0, x0]
    with pytest.raises(AssertionError, match="cell -> the point"):
        N.check_records(nodes, pts, 0.05, planted(R, cell_idx=idx), CAM)
    grid = R["grid"].copy()
    c = y0 * CAM[0] + x0
    grid[c, 3] = np.array([int(R["cell_idx"][y1, x1])], np.int32).view(np.float32)[0]
    with pytest.raises(AssertionError, match="grid"):
        N.check_records(nodes, pts, 0.05, planted(R, grid=grid), CAM)
    # two points in one cell, a point outside the image: not usable
    for p in (np.concatenate([pts, pts[:1] * np.float32(1.0001)]), np.concatenate([pts, [[1.0, 0.0, 0.4]]]).astype(np.float32)):
        assert not N.build_grid(p, CAM)[0]


def test_comb_tree_has_more_than_eight_wide_levels_at_depth_24_or_less():
    nodes, pts, _ = N.comb_tree()
    t = N.Tree(nodes, pts)
    _, _, level = N.wide_topology(t)
    assert t.depth <= 24 and level.max() + 1 > 8 and len(nodes) < 400
    assert level.max() + 1 > 16                                      # three rounds of eight levels
    assert np.all(t.size[~t.leaf] >= np.finfo(np.float32).tiny) and len(np.unique(t.size[~t.leaf])) == (~t.leaf).sum()   # no underflow, no ties
    # a valid tree: children pairwise and after their parents, parents agree, the split inside the gap, bbox = hull
    it = np.flatnonzero(~t.leaf)
    assert np.all(t.c2[it] == t.c1[it] + 1) and t.children_follow()
    assert np.all(nodes["parent"][t.c1[it]] == it) and np.all(nodes["parent"][t.c2[it]] == it) and nodes["parent"][0] == -1
    assert np.array_equal(t.box_lo, t.hull_lo) and np.array_equal(t.box_hi, t.hull_hi)
    assert np.all(t.hull_hi[t.c1[it], 0] < nodes["split_v"][it]) and np.all(nodes["split_v"][it] < t.hull_lo[t.c2[it], 0])
    rep = N.check_records(nodes, pts, 0.1, N.build_records(nodes, pts, 0.1))
    assert rep["continued"] and rep["wide_usable"] == 1


def test_forty_thousand_points_cross_the_chunk_seam():
    nodes, pts, _ = N.host_tree(N.random_points(40000, 4), 1)
    _, _, level = N.wide_topology(N.Tree(nodes, pts))
    sizes = N.level_sizes(level)
    assert any(s > N.K_WIDE_CHUNK and s % N.K_WIDE_CHUNK for s in sizes), sizes


def test_far_cases_fall_on_both_sides_of_the_frame_test():
    ok = {}
    for kind in ("far40", "far60"):
        f = nn_ref.degenerate(kind)
        nodes, pts, _ = N.host_tree(f.pts, f.max_leaf)
        ok[kind] = nn_ref.wide_frame_ok(nodes, f.max_dist)
        assert N.frames(N.Tree(nodes, pts), f.max_dist)[4] == ok[kind]
    assert ok == {"far40": True, "far60": False}


def test_record_layout():
    """A wide line written by hand as nn_wide_layout_kernel documents it: two halves of {two pairs of six words, first slot | second
    slot << 16, then four references}."""
    box = np.arange(48).reshape(1, 8, 6) + 100
    ref = np.array([[7, 8, 9, 10, 11, 12, 13, N.K_WIDE_EMPTY]])
    line = np.zeros(32, np.uint32)
    for h in range(2):
        for pr in range(2):
            for f in range(6):
                line[16 * h + 6 * pr + f] = box[0, 4 * h + 2 * pr, f] | (box[0, 4 * h + 2 * pr + 1, f] << 16)
        line[16 * h + 12:16 * h + 16] = ref[0, 4 * h:4 * h + 4]
    b, r = N.unpack_wide(line[None])
    assert np.array_equal(b, box) and np.array_equal(r, ref) and np.array_equal(N.pack_wide(box, ref)[0], line)
    assert C.sizeof(_lib.NNRecordsCounts) == 32 and C.sizeof(_lib.NNRecordsOut) == 11 * C.sizeof(C.c_void_p)
    assert N.grid_cells(97, 61) == 97 * 61 + 25 * 16 + 7 * 4 + 2 * 1
    # fma32 rounds once: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 midpoint, and an addend of 2^-100 either way decides (float64 loses it)
    x, lo, up = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -11), np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert N.fma32(x, x, np.float32(2.0 ** -100)) == up and N.fma32(x, x, np.float32(-2.0 ** -100)) == lo
    assert N.fma32(np.float32(3), np.float32(0.1), np.float32(7)) == np.float32(3 * float(np.float32(0.1)) + 7)


def test_entry_fails_loudly_without_gpu():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    d = _lib.SceneNNDesc(0.1, 16, 16, 16, 1, 1, 0, 0, 0, 0, 0, 0, 0)
    cnt = _lib.NNRecordsCounts()
    assert _lib.load().pr_debug_nn_records(C.addressof(d), 0, 0, None, C.byref(cnt), None) == _lib.PR_ERR_NO_DEVICE
    assert cnt.n_nodes == 0
