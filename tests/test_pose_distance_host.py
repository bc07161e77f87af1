"""Host side of the pose distances (no GPU): the record's layout, the numpy reference of pr_pose_distance (tests/pose_dist_ref.py) against a
float64 evaluation of the same definition, the argument checks -- which come before any device use, so they answer on a box without one --,
pr_cluster_greedy against its rule in Python, and symmetry_rotations."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_dist_ref as R
from pose_refine_amd import _lib, api, synth

K = synth.K_TEST


@pytest.fixture(scope="module")
def vertices(golden_dir):
    v = api.Model(os.path.join(golden_dir, "obj_06.ply")).vertices
    assert v.shape == (15736, 3) and len(np.unique(v, axis=0)) == len(v)
    return v


def test_record_layout_and_chunk_constant():
    d = _lib.POSE_DIST
    assert d.itemsize == 32
    assert [d.fields[n][1] for n in ("disp_sum_q16", "max_disp_sq", "max_proj_sq", "sym_sum", "sym_disp", "sym_proj", "reserved", "n_points", "reserved2")] == \
        [0, 8, 12, 16, 18, 20, 22, 24, 28]
    assert api.get_option("pose_dist_chunk") == _lib.POSE_DIST_CHUNK
    assert "pr_pose_distance" in _lib.SIGNATURES and "pr_cluster_greedy" in _lib.SIGNATURES


def test_reference_against_float64(vertices):
    """The mean within half a quantum plus eight float32 rounding units on the magnitude of the terms (the worst case measured is 0.04 of that
    bound), the maximum within a relative 1e-6 (1.5e-7 measured), the projection within 1e-3 px (5e-5 measured)."""
    gt = synth.scene_pose()
    hyps = synth.hypotheses(200)[1::5]
    syms = api.symmetry_rotations((0, 0, 1), 7)
    n = len(vertices)
    worst = [0.0, 0.0, 0.0]
    for A in hyps:
        rec, cands = R.record(vertices, A, gt, syms, K, per_candidate=True)
        for k, (total, maxd, maxp) in enumerate(cands):
            mean64, max64, px64, mag = R.truth64(vertices, A, gt, syms[k], K)
            bound = 2.0 ** -17 + 8 * 2.0 ** -24 * mag
            e_mean = abs(total / 65536.0 / n - mean64)
            e_max = abs(np.sqrt(np.float64(maxd)) - max64) / max64
            e_px = abs(np.sqrt(np.float64(maxp)) - px64)
            worst = [max(worst[0], e_mean / bound), max(worst[1], e_max), max(worst[2], e_px)]
            assert e_mean <= bound and e_max <= 1e-6 and e_px <= 1e-3, (k, e_mean, bound, e_max, e_px)
        # the record is the three minima, each on its own
        assert rec["disp_sum_q16"] == min(c[0] for c in cands) and rec["max_disp_sq"] == min(c[1] for c in cands)
        assert rec["max_proj_sq"] == min(c[2] for c in cands) and rec["n_points"] == n
    print("worst: mean error / bound %.3g, max relative %.3g, projection %.3g px" % tuple(worst))


def test_reference_identical_and_tiny_shift(vertices):
    syms = api.symmetry_rotations((0, 0, 1), 7)
    A = synth.hypotheses(4)[3]
    rec = R.record(vertices, A, A, syms, K)
    want = np.zeros((), _lib.POSE_DIST)
    want["n_points"] = len(vertices)
    assert rec.tobytes() == want.tobytes()
    B = A.copy()
    B[0, 3] += np.float32(0.002)
    rec = R.record(vertices, A, B)
    mean = rec["disp_sum_q16"] / 65536.0 / len(vertices)
    assert abs(mean - 0.002) <= 2.0 ** -16
    assert api.mean_displacement(rec) == mean
    assert abs(api.max_displacement(rec) - 0.002) <= 1e-6 and api.max_projection(rec) == 0.0


# ---- argument checks: before any device is touched ---------------------------------------------------------------------------------
FAKE_DEV = 0x10000                       # a non-null "device pointer" that a correct library never dereferences in these calls


def _call(points=FAKE_DEV, n_points=10, a="eye", n_a=None, b="eye", n_b=None, all_pairs=0, syms=None, n_syms=None, Kc=None, out="buf"):
    """pr_pose_distance on four identity poses a side unless told otherwise (None: a null pointer); nothing may be written unless it succeeds."""
    eye = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    a = eye if isinstance(a, str) else a
    b = eye if isinstance(b, str) else b
    buf = np.full(16 * 32, 0xAB, np.uint8)
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)  # noqa: E731
    n = lambda x, given: given if given is not None else (0 if x is None else len(x))  # noqa: E731
    rc = _lib.load().pr_pose_distance(points, n_points, p(a), n(a, n_a), p(b), n(b, n_b), all_pairs, p(syms), n(syms, n_syms), p(Kc),
                                      buf.ctypes.data if out == "buf" else out)
    assert (buf == 0xAB).all() or rc == _lib.PR_OK
    return rc


def test_invalid_arguments_are_rejected_before_any_device_use():
    INV = _lib.PR_ERR_INVALID
    eye = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    big = np.tile(np.eye(4, dtype=np.float32), (_lib.POSE_DIST_MAX_POSES + 1, 1, 1))
    many = np.tile(np.eye(4, dtype=np.float32), (_lib.POSE_DIST_MAX_SYMS + 1, 1, 1))
    assert _call(n_points=0) == INV
    assert _call(n_points=_lib.POSE_DIST_MAX_POINTS + 1) == INV
    assert _call(a=big, b=big) == INV
    assert _call(a=big, all_pairs=1) == INV and _call(b=big, all_pairs=1) == INV
    assert _call(a=big, n_a=len(big), b=eye, n_b=0, all_pairs=1) == INV        # a cap holds even with nothing to compute
    assert _call(syms=many) == INV
    assert _call(a=eye[:3], b=eye) == INV                                       # pair mode: as many of each
    assert _call(a=eye[:3], b=eye[:0]) == INV
    assert _call(points=None) == INV and _call(a=None, n_a=4) == INV and _call(b=None, n_b=4) == INV and _call(out=None) == INV
    assert _call(syms=None, n_syms=3) == INV                                    # symmetries announced, none given
    for bad in (np.nan, np.inf, -np.inf):
        for where in ("a", "b", "syms", "K"):
            m = eye.copy()
            m[2, 1, 3] = bad
            kc = K.copy()
            if where == "K":
                kc[7] = bad                                                     # an entry the projection never reads: every entry is checked
            rc = _call(a=m if where == "a" else "eye", b=m if where == "b" else "eye", syms=m if where == "syms" else None, Kc=kc)
            assert rc == INV, (bad, where)
            assert "pr_pose_distance" in _lib.load().pr_last_error().decode()
    for i in (0, 4):
        kc = K.copy()
        kc[i] = 0.0
        assert _call(Kc=kc) == INV
    # nothing to compute: PR_OK without a device, without arrays
    lib = _lib.load()
    assert lib.pr_pose_distance(None, 0, None, 0, None, 0, 0, None, 0, None, None) == _lib.PR_OK
    assert lib.pr_pose_distance(None, 0, eye.ctypes.data, 4, None, 0, 1, None, 0, None, None) == _lib.PR_OK
    assert lib.pr_pose_distance(None, 0, None, 0, eye.ctypes.data, 4, 1, None, 0, K.ctypes.data, None) == _lib.PR_OK
    if api.device_count() == 0:                                                 # ... and a valid call does ask for the device
        assert _call() == _lib.PR_ERR_NO_DEVICE and _call(all_pairs=1, Kc=K, syms=eye) == _lib.PR_ERR_NO_DEVICE
        with pytest.raises(api.PoseRefineError) as e:
            api.pose_distance(np.zeros((5, 3), np.float32), eye, eye)
        assert e.value.code == _lib.PR_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        api.pose_distance(np.zeros((5, 3), np.float32), eye, eye[:3])
    with pytest.raises(ValueError):
        api.pose_distance(np.zeros((5, 3), np.float32), eye, np.zeros((2, 3, 4), np.float32))


# ---- pr_cluster_greedy --------------------------------------------------------------------------------------------------------------
def _random_dist(rng, P, radius):
    """A distance matrix as an all_pairs call could return it, but not symmetric: entries around the radius, exact ties at it, and pairs
    where only one direction lies within it."""
    r2 = np.float32(radius) * np.float32(radius)
    d2 = (rng.random((P, P)) ** 2 * 6.0 * r2).astype(np.float32)
    d2 = np.minimum(d2, d2.T)                                    # symmetric to start with
    tie = rng.random((P, P)) < 0.05
    d2[tie] = r2                                                 # exactly at the radius: <= keeps the pair together
    one_way = np.triu(rng.random((P, P)) < 0.1, 1)
    d2[one_way] = r2 * np.float32(3.0)                           # [i][j] outside ...
    d2.T[one_way] = np.minimum(d2.T[one_way], r2 * np.float32(0.5))     # ... [j][i] inside
    d2[np.arange(P), np.arange(P)] = 0.0
    dist = np.zeros((P, P), _lib.POSE_DIST)
    dist["max_disp_sq"] = d2
    dist["disp_sum_q16"] = rng.integers(0, 1 << 40, (P, P))      # fields the rule must not look at
    dist["max_proj_sq"] = rng.random((P, P))
    return dist


@pytest.mark.parametrize("P", [1, 2, 17, 100, 300])
@pytest.mark.parametrize("radius", [0.0, 0.5, 1.0, 2.5])
def test_cluster_greedy_matches_reference(P, radius):
    rng = np.random.default_rng(1000 * P + int(radius * 10))
    dist = _random_dist(rng, P, radius if radius > 0 else 1.0)
    for order in (rng.permutation(P), rng.permutation(P)[:max(1, P // 3)]):          # a full and a partial order
        kept, rep = api.merge_duplicates(order, dist, radius)
        want_kept, want_rep = R.cluster_greedy(order, dist, radius)
        assert kept.dtype == np.int64 and kept.tolist() == want_kept
        assert rep.tolist() == want_rep.tolist()
        assert set(np.flatnonzero(rep >= 0).tolist()) == set(int(i) for i in order)
        assert all(rep[i] == i for i in kept) and set(rep[rep >= 0].tolist()) == set(kept.tolist())


def test_cluster_greedy_ties_and_one_way_entries():
    dist = np.zeros((2, 2), _lib.POSE_DIST)
    dist["max_disp_sq"] = [[0, 2.25], [2.25, 0]]
    assert api.merge_duplicates([0, 1], dist, 1.5)[0].tolist() == [0]             # exactly at the radius: the same pose
    assert api.merge_duplicates([1, 0], dist, 1.5)[0].tolist() == [1]
    dist["max_disp_sq"] = [[0, np.nextafter(np.float32(2.25), np.float32(3))], [np.nextafter(np.float32(2.25), np.float32(3)), 0]]
    assert api.merge_duplicates([0, 1], dist, 1.5)[0].tolist() == [0, 1]          # one float beyond: two poses
    dist["max_disp_sq"] = [[0, 100.0], [1.0, 0]]                                   # only [1][0] within the radius
    for order in ([0, 1], [1, 0]):
        kept, rep = api.merge_duplicates(order, dist, 1.5)
        assert kept.tolist() == order[:1] and rep.tolist() == [order[0], order[0]]
    dist["max_disp_sq"] = [[0, np.inf], [np.nan, 0]]
    assert api.merge_duplicates([0, 1], dist, 1e18)[0].tolist() == [0, 1]         # inf and NaN are never within a radius
    # the absorbing hypothesis is the first in kept order that is near, not the nearest
    d3 = np.zeros((3, 3), _lib.POSE_DIST)
    d3["max_disp_sq"] = [[0, 50, 0.9], [50, 0, 0.1], [0.9, 0.1, 0]]
    kept, rep = api.merge_duplicates([0, 1, 2], d3, 1.0)
    assert kept.tolist() == [0, 1] and rep.tolist() == [0, 1, 0]


def _cluster_raw(order, dist, n_poses, radius, rep=True):
    order = np.ascontiguousarray(order, np.uint32)
    kept = np.full(max(1, len(order)), 0xffffffff, np.uint32)
    reps = np.full(max(1, n_poses), 0xffffffff, np.uint32)
    n = C.c_uint32(12345)
    rc = _lib.load().pr_cluster_greedy(order.ctypes.data, len(order), dist.ctypes.data, n_poses, radius, kept.ctypes.data, C.byref(n),
                                       reps.ctypes.data if rep else None)
    return rc, kept, n.value, reps


def test_cluster_greedy_invalid_arguments_and_null_rep():
    dist = _random_dist(np.random.default_rng(2), 6, 1.0)
    for order in ([0, 1, 6], [0, 1, 1], [5, 4, 5, 3], [4294967295]):
        rc, kept, n, reps = _cluster_raw(order, dist, 6, 1.0)
        assert rc == _lib.PR_ERR_INVALID, order
        assert (kept == 0xffffffff).all() and (reps == 0xffffffff).all() and n == 12345      # nothing written
        with pytest.raises(api.PoseRefineError) as e:
            api.merge_duplicates(order, dist, 1.0)
        assert e.value.code == _lib.PR_ERR_INVALID and "pr_cluster_greedy" in str(e.value)
    for radius in (-1.0, -0.0001, np.nan, np.inf, -np.inf):
        rc, kept, n, reps = _cluster_raw([0, 1, 2], dist, 6, radius)
        assert rc == _lib.PR_ERR_INVALID, radius
        assert (kept == 0xffffffff).all() and (reps == 0xffffffff).all() and n == 12345
    # rep_out == NULL: the kept list alone
    order = [3, 0, 5, 1, 2, 4]
    rc, kept, n, _ = _cluster_raw(order, dist, 6, 1.0, rep=False)
    assert rc == _lib.PR_OK and kept[:n].tolist() == R.cluster_greedy(order, dist, 1.0)[0]
    lib = _lib.load()
    od, out = np.arange(3, dtype=np.uint32), np.zeros(3, np.uint32)
    assert lib.pr_cluster_greedy(od.ctypes.data, 3, dist.ctypes.data, 6, 1.0, out.ctypes.data, None, None) == _lib.PR_ERR_INVALID
    assert lib.pr_cluster_greedy(None, 3, dist.ctypes.data, 6, 1.0, out.ctypes.data, C.byref(C.c_uint32()), None) == _lib.PR_ERR_INVALID
    assert lib.pr_cluster_greedy(od.ctypes.data, 3, None, 6, 1.0, out.ctypes.data, C.byref(C.c_uint32()), None) == _lib.PR_ERR_INVALID
    assert lib.pr_cluster_greedy(od.ctypes.data, 3, dist.ctypes.data, 6, 1.0, None, C.byref(C.c_uint32()), None) == _lib.PR_ERR_INVALID
    n = C.c_uint32(7)
    assert lib.pr_cluster_greedy(None, 0, None, 0, 1.0, None, C.byref(n), None) == _lib.PR_OK and n.value == 0
    with pytest.raises(ValueError):
        api.merge_duplicates([0, 1], dist[:, :5], 1.0)
    with pytest.raises(ValueError):
        api.merge_duplicates([0, -1], dist, 1.0)


# ---- symmetry_rotations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,n,center", [((0, 0, 1), 7, (0, 0, 0)), ((1, 2, -0.5), 5, (0.5, -0.25, 0.125)), ((0, 3, 0), 2, (1, 1, 1)),
                                           ((1, 1, 1), 8, (0, 0, 0)), ((0, 0, -2), 1, (0.5, 0.5, 0.5))])
def test_symmetry_rotations(axis, n, center):
    S = api.symmetry_rotations(axis, n, center)
    assert S.shape == (n, 4, 4) and S.dtype == np.float32
    assert np.array_equal(S[0], np.eye(4, dtype=np.float32))
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    for k in range(n):
        Sk = S[k].astype(np.float64)
        assert np.abs(np.linalg.matrix_power(Sk, n) - np.eye(4)).max() <= 1e-6
        assert np.abs(Sk[:3, :3] @ ax - ax).max() <= 1e-6 and np.array_equal(S[k, 3], [0, 0, 0, 1])
        assert np.abs(Sk[:3, :3] @ Sk[:3, :3].T - np.eye(3)).max() <= 1e-6
    with pytest.raises(ValueError):
        api.symmetry_rotations((0, 0, 0), 3)
    with pytest.raises(ValueError):
        api.symmetry_rotations((0, 0, 1), 0)


def test_symmetry_rotations_about_a_centre_off_the_origin():
    """Every entry is a float64 value rounded once (relative 2^-24), so S c - c is at most 2^-24 (sum_j |r_ij| |c_j| + |t_i|) per row:
    below 2^-24 * 8 * max|c| for a rotation."""
    c = np.array([10.0, -20.0, 35.5])
    S = api.symmetry_rotations((1, 2, -0.5), 6, c)
    for k in range(6):
        Sk = S[k].astype(np.float64)
        assert np.abs(Sk @ np.append(c, 1.0) - np.append(c, 1.0)).max() <= 2.0 ** -24 * 8 * 35.5
        if k:
            assert np.abs(Sk[:3, 3]).max() > 1.0                                 # (the centre is not on the axis through the origin)
    assert np.abs(S[1].astype(np.float64) @ S[5].astype(np.float64) - np.eye(4)).max() <= 2.0 ** -24 * 16 * 35.5
