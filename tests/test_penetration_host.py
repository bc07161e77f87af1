"""Host side of the interpenetration check (no GPU): the numpy restatement of the raster pinned to the oracle, the definition on two boxes
whose answer is known in closed form, pr_select_disjoint against the walk in Python integers, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from gpu_common import pathological_hypotheses
from pose_refine_amd import _lib, api, synth
from solid_ref import (PLANTED_KEPT, box_mesh, check_invariants, disjoint_ref, pairs_ref, planted, span_ref)

W, H = synth.WIDTH, synth.HEIGHT
ROIS = [(200, 150, 200, 180), (0, 100, 330, 200)]                  # two of test_select_gpu.py's list


# ---- 1. the reference is pinned by the oracle -------------------------------------------------------------------------------------------
def test_min_composite_is_the_oracle_render(scenario):
    poses = synth.hypotheses(16)
    near, far = span_ref(scenario["tris"], poses, scenario["proj"], W, H)
    assert np.array_equal(near, O.render(scenario["tris"], poses, W, H, scenario["proj"]))
    drawn = near > 0
    assert drawn.sum() > 16 * 5000 and (far[drawn] >= near[drawn]).all() and not far[~drawn].any()
    assert (far[drawn] > near[drawn]).mean() > 0.9                  # a closed mesh: almost every pixel has a back surface behind the front one


@pytest.mark.parametrize("roi", ROIS)
def test_min_composite_is_the_oracle_render_roi(scenario, roi):
    poses = synth.hypotheses(16)[:6]
    near, far = span_ref(scenario["tris"], poses, scenario["proj"], W, H, roi)
    assert near.shape == (6, roi[3], roi[2])
    assert np.array_equal(near, O.render(scenario["tris"], poses, W, H, scenario["proj"], roi))
    # the window of the full-frame planes: a ROI clips fragments, it does not change them
    full_near, full_far = span_ref(scenario["tris"], poses, scenario["proj"], W, H)
    x, y, w, h = roi
    assert np.array_equal(near, full_near[:, y:y + h, x:x + w]) and np.array_equal(far, full_far[:, y:y + h, x:x + w])


def test_min_composite_is_the_oracle_render_pathological(scenario):
    """NaN / infinite / zero matrices, mirrored, the camera inside the object, behind it, a giant, a speck: f2i_x86 and loop_start decide."""
    bad, idx_bad = pathological_hypotheses(synth.hypotheses(24))
    near, _ = span_ref(scenario["tris"], bad, scenario["proj"], W, H)
    ora = O.render(scenario["tris"], bad, W, H, scenario["proj"])
    for i in range(len(bad)):
        assert np.array_equal(near[i], ora[i]), i
    assert sum(bool(ora[i].any()) for i in idx_bad) >= 4            # some of them do draw: the comparison is not one of empty frames


# ---- 2. the definition on two boxes ---------------------------------------------------------------------------------------------------
# fx = fy = 460 and a principal point half a pixel off the grid: a face of half-width s at depth z ends 460 s / z pixels from x = 32.5.  Under perspective a
# ray near the silhouette leaves a box through a side face; the half-widths (3 and 4 mm) are chosen so that no pixel centre lies in those rings
# (box 1: 3.0 .. 3.45 px, box 2: 3.54 .. 4.18 px from the axis), so every covered pixel sees a front and a back face and the thickness is the depth extent.
BW, BH = 64, 48
BOX_K = np.array([460, 0, 32.5, 0, 460, 24.5, 0, 0, 1], np.float32)


def _z_pose(z):
    p = np.eye(4, dtype=np.float32)
    p[2, 3] = z
    return p


def _box_planes(z0, z1, half):
    proj = O.compute_proj(BOX_K, BW, BH)
    return span_ref(box_mesh(half, half, (z1 - z0) / 2), _z_pose((z0 + z1) / 2)[None], proj, BW, BH, raw=True)


@pytest.mark.parametrize("second, overlap", [((440, 520), 20), ((470, 520), 0)])
def test_two_boxes_in_closed_form(second, overlap):
    n1, f1 = _box_planes(400, 460, 3.0)
    n2, f2 = _box_planes(*second, 4.0)
    near, far = np.concatenate([n1, n2]), np.concatenate([f1, f2])
    d1, d2 = n1[0] != np.iinfo(np.int32).max, n2[0] != np.iinfo(np.int32).max
    assert d1.sum() == 36 and d2.sum() == 64 and (d1 & d2).sum() == 36          # 6 x 6 and 8 x 8 pixels about the axis
    assert (n1[0][d1] == 400).all() and (f1[0][d1] == 460).all() and (n2[0][d2] == second[0]).all() and (f2[0][d2] == second[1]).all()
    both = d1 & d2
    ln = np.minimum(f1[0], f2[0]).astype(np.int64) - np.maximum(n1[0], n2[0])
    assert (ln[both] == 460 - second[0]).all()                    # every pixel both cover: 20, or -10 for the box that keeps its distance
    p0 = pairs_ref(near, far, 0)
    check_invariants(p0)
    assert p0["both"].tolist() == [[36, 36], [36, 64]]
    assert p0["sum_mm"][0, 0] == 60 * 36 and p0["sum_mm"][1, 1] == (second[1] - second[0]) * 64      # the diagonal: 60 and 80 (50) per pixel
    assert p0["max_mm"][0, 0] == 60 and p0["max_mm"][1, 1] == second[1] - second[0]
    if overlap:
        for slack in (0, 19):
            p = pairs_ref(near, far, slack)
            assert p["inter"][0, 1] == p["both"][0, 1] == 36 and p["sum_mm"][0, 1] == 20 * 36 and p["max_mm"][0, 1] == 20
        p = pairs_ref(near, far, 20)
        assert p["inter"][0, 1] == 0 and p["sum_mm"][0, 1] == 0 and p["max_mm"][0, 1] == 0 and p["both"][0, 1] == 36
        assert api.penetration_fraction(p0)[0, 1] == 20 / 60
    else:
        assert p0["inter"][0, 1] == 0 and p0["sum_mm"][0, 1] == 0 and p0["both"][0, 1] == 36
        assert api.penetration_fraction(p0)[0, 1] == 0.0


# ---- 3. pr_select_disjoint through the C ABI ----------------------------------------------------------------------------------------------
def _random_pairs(rng, P, top):
    """A symmetric matrix that could be the device's: sum[i][j] <= min of the two diagonal sums."""
    diag = rng.integers(0, top, P, dtype=np.uint64)
    diag[rng.random(P) < 0.1] = 0
    lim = np.minimum(diag[:, None], diag[None, :])
    share = (rng.random((P, P)) ** 3 * lim.astype(np.float64)).astype(np.uint64)
    share[rng.random((P, P)) < 0.4] = 0
    share = np.minimum(np.triu(share, 1) + np.triu(share, 1).T, lim)
    share[np.arange(P), np.arange(P)] = diag
    out = np.zeros((P, P), api.PAIR_SOLID)
    out["sum_mm"] = share
    out["inter"] = (share > 0)
    out["both"] = out["inter"]
    return out


def _disjoint_raw(order, pairs, num, den, n_poses=None):
    order = np.ascontiguousarray(order, np.uint32)
    pairs = np.ascontiguousarray(pairs, api.PAIR_SOLID)
    sel = np.full(max(1, len(order)), 0xffffffff, np.uint32)
    n = C.c_uint32(12345)
    rc = _lib.load().pr_select_disjoint(order.ctypes.data, len(order), pairs.ctypes.data, len(pairs) if n_poses is None else n_poses, num, den,
                                        sel.ctypes.data, C.byref(n))
    return rc, sel, n.value


def test_disjoint_matches_reference_on_random_matrices():
    rng = np.random.default_rng(77)
    fracs = [(0, 1), (1, 10), (1, 4), (1, 2), (1, 1), (7, 3), (4294967295, 4294967295), (1, 4294967295)]
    dropped = 0
    for case in range(200):
        P = int(rng.integers(1, 41))
        pairs = _random_pairs(rng, P, 1 << int(rng.integers(4, 40)))
        order = rng.permutation(P)[:int(rng.integers(1, P + 1))]
        num, den = fracs[case % len(fracs)]
        got = api.select_disjoint(order, pairs, (num, den))
        want = disjoint_ref(order, pairs, num, den)
        assert got.dtype == np.int64 and got.tolist() == want, case
        dropped += len(order) - len(want)
        if num >= den:                                           # shared <= min always: everything survives
            assert want == [int(i) for i in order]
    assert dropped > 200                                          # the rule is exercised


def test_disjoint_needs_128_bit_products():
    """sum_mm near 2^57 against den near 2^32: the products reach 2^89.  A 64-bit product wraps and decides the other way."""
    big = (1 << 57) - 12345
    pairs = np.zeros((2, 2), api.PAIR_SOLID)
    pairs["sum_mm"] = [[big, big // 2 + 7], [big // 2 + 7, big]]
    den = (1 << 32) - 5
    for num in (den // 2, den // 2 + 1, 1, den - 1):
        assert ((big // 2 + 7) * den) % (1 << 64) != (big // 2 + 7) * den          # it does wrap in 64 bits
        want = disjoint_ref([0, 1], pairs, num, den)
        assert api.select_disjoint([0, 1], pairs, (num, den)).tolist() == want
    assert disjoint_ref([0, 1], pairs, den // 2, den) == [0] and disjoint_ref([0, 1], pairs, den // 2 + 1, den) == [0, 1]
    # a tie at the bound is not a conflict, one more millimetre is
    tie = np.zeros((2, 2), api.PAIR_SOLID)
    tie["sum_mm"] = [[1 << 56, 1 << 54], [1 << 54, 1 << 57]]
    assert api.select_disjoint([0, 1], tie, (1 << 29, 1 << 31)).tolist() == [0, 1]
    tie["sum_mm"][0, 1] = tie["sum_mm"][1, 0] = (1 << 54) + 1
    assert api.select_disjoint([0, 1], tie, (1 << 29, 1 << 31)).tolist() == [0]
    assert api.select_disjoint([1, 0], tie, (1 << 29, 1 << 31)).tolist() == [1]
    # without volume: never a conflict, and kept
    flat = np.zeros((3, 3), api.PAIR_SOLID)
    flat["sum_mm"][1, 1] = 500
    assert api.select_disjoint([0, 1, 2], flat, (0, 1)).tolist() == [0, 1, 2]


def test_disjoint_invalid_arguments():
    pairs = _random_pairs(np.random.default_rng(1), 6, 1000)
    for order in ([0, 1, 6], [0, 1, 1], [5, 4, 5, 3], [4294967295]):
        rc, sel, n = _disjoint_raw(order, pairs, 1, 10)
        assert rc == _lib.PR_ERR_INVALID, order
        assert (sel == 0xffffffff).all() and n == 12345          # nothing written
        with pytest.raises(api.PoseRefineError) as e:
            api.select_disjoint(order, pairs, (1, 10))
        assert e.value.code == _lib.PR_ERR_INVALID and "pr_select_disjoint" in str(e.value)
    rc, sel, n = _disjoint_raw([0, 1, 2], pairs, 1, 0)
    assert rc == _lib.PR_ERR_INVALID and (sel == 0xffffffff).all() and n == 12345
    with pytest.raises(api.PoseRefineError) as e:
        api.select_disjoint([0, 1], pairs, (0, 0))
    assert "den" in str(e.value)
    lib = _lib.load()
    od, out = np.arange(3, dtype=np.uint32), np.zeros(3, np.uint32)
    assert lib.pr_select_disjoint(od.ctypes.data, 3, pairs.ctypes.data, 6, 1, 10, out.ctypes.data, None) == _lib.PR_ERR_INVALID
    assert lib.pr_select_disjoint(None, 3, pairs.ctypes.data, 6, 1, 10, out.ctypes.data, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    assert lib.pr_select_disjoint(od.ctypes.data, 3, None, 6, 1, 10, out.ctypes.data, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    assert lib.pr_select_disjoint(od.ctypes.data, 3, pairs.ctypes.data, 6, 1, 10, None, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    n = C.c_uint32(7)
    assert lib.pr_select_disjoint(None, 0, None, 0, 1, 10, None, C.byref(n)) == _lib.PR_OK and n.value == 0
    with pytest.raises(ValueError):
        api.select_disjoint([0, 1], pairs[:, :5], (1, 10))       # not square
    with pytest.raises(ValueError):
        api.select_disjoint([0, -1], pairs, (1, 10))


def test_planted_set_on_the_cpu(scenario):
    """S, two poses sunk into it, one 120 mm behind it, one beside it: the rule 1/10 keeps [0, 2, 3].  The pair (S, behind) shares thousands of pixels and no
    volume -- the case the pixel rules cannot tell from a conflict.  Counts and fractions as measured when the check was proposed."""
    near, far = span_ref(scenario["tris"], planted(), scenario["proj"], W, H, raw=True)
    pairs = pairs_ref(near, far, 0)
    check_invariants(pairs)
    assert pairs["both"][0, 2] > 0 and pairs["inter"][0, 2] == 0
    assert pairs["both"][0].tolist()[1:] == [18107, 10796, 0, 13277]
    frac = api.penetration_fraction(pairs)
    assert np.round(frac[0], 3).tolist() == [1.0, 0.760, 0.0, 0.0, 0.470]
    assert np.array_equal(frac, frac.T) and (np.diag(frac) == 1.0).all()
    assert api.select_disjoint(np.arange(5), pairs).tolist() == PLANTED_KEPT == disjoint_ref(range(5), pairs, 1, 10)
    assert api.select_disjoint([4, 3, 2, 1, 0], pairs).tolist() == [4, 3, 2]      # the order decides which of a conflicting pair stays


# ---- 4. refusals, with no device ----------------------------------------------------------------------------------------------------------
def _penetration_raw(n_poses, width, height, slack, multi=False):
    lib = _lib.load()
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (max(1, n_poses), 1))
    pj = np.eye(4, dtype=np.float32)
    out = np.full((2, 2), 0x5a, np.uint8)                         # (refused before anything is written: never sized for the batch)
    if multi:
        table, idx = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0)), np.zeros(max(1, n_poses), np.uint32)
        rc = lib.pr_pose_penetration_multi(table, 1, idx.ctypes.data, poses.ctypes.data, n_poses, width, height, pj.ctypes.data, slack, out.ctypes.data)
    else:
        rc = lib.pr_pose_penetration(None, 0, poses.ctypes.data, n_poses, width, height, pj.ctypes.data, slack, out.ctypes.data)
    assert (out == 0x5a).all()
    return rc, lib.pr_last_error().decode()


@pytest.mark.parametrize("multi", [False, True])
def test_refusals_need_no_device(multi):
    name = "pr_pose_penetration_multi" if multi else "pr_pose_penetration"
    rc, msg = _penetration_raw(4, 640, 480, -1, multi)
    assert rc == _lib.PR_ERR_INVALID and name in msg and "-1" in msg
    rc, msg = _penetration_raw(1025, 64, 48, 0, multi)
    assert rc == _lib.PR_ERR_INVALID and name in msg and "1025" in msg and "1024" in msg
    rc, msg = _penetration_raw(64, 4096, 4096, 0, multi)          # 128 renders of 64 MiB each: twice what the depth workspace holds
    assert rc == _lib.PR_ERR_INVALID and name in msg and "128" in msg and "64" in msg and "4096x4096" in msg
    rc, msg = _penetration_raw(32, 4096, 4096, -5, multi)
    assert rc == _lib.PR_ERR_INVALID and "-5" in msg
    rc, msg = _penetration_raw(4, 0, 480, 0, multi)
    assert rc == _lib.PR_ERR_INVALID
    rc, msg = _penetration_raw(4, 8193, 16, 0, multi)
    assert rc == _lib.PR_ERR_INVALID and "8193" in msg
    rc, _ = _penetration_raw(0, 640, 480, 0, multi)               # nothing to do: no device needed either
    assert rc == _lib.PR_OK
    assert api.PENETRATION_MAX_POSES == 1024


def test_device_calls_without_gpu_fail_loudly():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    lib = _lib.load()
    pose, pj = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    out = np.zeros(1, api.PAIR_SOLID)
    assert lib.pr_pose_penetration(None, 0, pose.ctypes.data, 1, 64, 48, pj.ctypes.data, 0, out.ctypes.data) == _lib.PR_ERR_NO_DEVICE
    assert lib.pr_render_span(None, 0, None, 0, 64, 48, pj.ctypes.data, _lib.Roi(0, 0, 0, 0), None, None) == _lib.PR_ERR_NO_DEVICE
