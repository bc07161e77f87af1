"""Host side of detection selection (no GPU): pr_select_greedy against the rule in Python integers, select_hypotheses' use of the ranking,
the no-device error of the device calls, and the planted frame end to end on the CPU (oracle renders -> score_ref -> overlap_ref)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from select_ref import (PLANTED_EXACT, PLANTED_SELECTION, greedy_ref, overlap_ref, planted_frame, rank_fraction)
from verify_ref import score_ref

W, H = synth.WIDTH, synth.HEIGHT


def _random_overlap(rng, P, zero_diag=0.1):
    """A symmetric matrix that could be an overlap matrix: shared <= min of the two diagonal entries."""
    diag = rng.integers(1, 5000, P)
    diag[rng.random(P) < zero_diag] = 0
    lim = np.minimum(diag[:, None], diag[None, :])
    share = (rng.random((P, P)) ** 3 * (lim + 1)).astype(np.int64)
    share[rng.random((P, P)) < 0.5] = 0
    share = np.minimum(np.triu(share, 1) + np.triu(share, 1).T, lim)
    share[np.arange(P), np.arange(P)] = diag
    return share.astype(np.uint32)


def _greedy_raw(order, ov, num, den, n_poses=None):
    order = np.ascontiguousarray(order, np.uint32)
    ov = np.ascontiguousarray(ov, np.uint32)
    sel = np.full(max(1, len(order)), 0xffffffff, np.uint32)
    n = C.c_uint32(12345)
    rc = _lib.load().pr_select_greedy(order.ctypes.data, len(order), ov.ctypes.data, len(ov) if n_poses is None else n_poses, num, den,
                                      sel.ctypes.data, C.byref(n))
    return rc, sel, n.value


@pytest.mark.parametrize("P", [1, 2, 17, 100, 300])
@pytest.mark.parametrize("frac", [(0, 1), (1, 10), (1, 4), (1, 2), (3, 4), (1, 1), (7, 3)])
def test_greedy_matches_reference(P, frac):
    rng = np.random.default_rng(100 * P + frac[0] * 13 + frac[1])
    ov = _random_overlap(rng, P)
    order = rng.permutation(P)
    got = api.select_greedy(order, ov, *frac)
    want = greedy_ref(order, ov, *frac)
    assert got.dtype == np.int64 and got.tolist() == want
    assert all(ov[i, i] > 0 for i in got)
    if frac == (0, 1):                                           # nothing may be shared at all
        assert all(ov[i, j] == 0 for a, i in enumerate(got) for j in got[:a])
    if frac[0] >= frac[1]:                                       # shared <= min always: everything with support survives
        assert got.tolist() == [int(i) for i in order if ov[i, i] > 0]


def test_greedy_partial_order_and_ties():
    rng = np.random.default_rng(4)
    ov = _random_overlap(rng, 120, zero_diag=0.0)
    order = rng.permutation(120)[:37]                            # a partial order: only its entries can be selected
    got = api.select_greedy(order, ov, 1, 4)
    assert got.tolist() == greedy_ref(order, ov, 1, 4) and set(got) <= set(order.tolist())
    # a tie at the bound: shared * den == num * min is NOT a conflict, one more shared pixel is
    tie = np.array([[100, 25], [25, 200]], np.uint32)
    assert api.select_greedy([0, 1], tie, 1, 4).tolist() == [0, 1]
    assert api.select_greedy([1, 0], tie, 1, 4).tolist() == [1, 0]
    tie[0, 1] = tie[1, 0] = 26
    assert api.select_greedy([0, 1], tie, 1, 4).tolist() == [0]
    assert api.select_greedy([1, 0], tie, 1, 4).tolist() == [1]
    # identical hypotheses: the first of the order wins
    same = np.full((5, 5), 77, np.uint32)
    assert api.select_greedy([3, 1, 4, 0, 2], same, 1, 2).tolist() == [3]
    # products beyond 32 bits: 4e9 * 4e9 must not wrap
    big = np.array([[4000000000, 3000000000], [3000000000, 4000000000]], np.uint32)
    assert api.select_greedy([0, 1], big, 3, 4).tolist() == [0, 1]
    assert api.select_greedy([0, 1], big, 2999999999, 4000000000).tolist() == [0]
    assert api.select_greedy([0, 1], big, 4294967295, 4294967295).tolist() == [0, 1]


def test_greedy_all_zero_diagonal_and_empty():
    ov = np.zeros((9, 9), np.uint32)
    ov[2, 5] = ov[5, 2] = 3                                      # (not a possible overlap matrix; the diagonal alone decides)
    assert api.select_greedy(np.arange(9), ov, 1, 4).tolist() == []
    assert api.select_greedy(np.zeros(0, np.int64), ov, 1, 4).tolist() == []
    n = C.c_uint32(7)
    assert _lib.load().pr_select_greedy(None, 0, None, 0, 1, 4, None, C.byref(n)) == _lib.PR_OK and n.value == 0


def test_greedy_invalid_arguments():
    ov = _random_overlap(np.random.default_rng(1), 6, zero_diag=0.0)
    for order in ([0, 1, 6], [0, 1, 1], [5, 4, 5, 3], [4294967295]):
        rc, sel, n = _greedy_raw(order, ov, 1, 4)
        assert rc == _lib.PR_ERR_INVALID, order
        assert (sel == 0xffffffff).all() and n == 12345          # nothing written
        with pytest.raises(api.PoseRefineError) as e:
            api.select_greedy(order, ov, 1, 4)
        assert e.value.code == _lib.PR_ERR_INVALID and "pr_select_greedy" in str(e.value)
    rc, sel, n = _greedy_raw([0, 1, 2], ov, 1, 0)
    assert rc == _lib.PR_ERR_INVALID and (sel == 0xffffffff).all() and n == 12345
    with pytest.raises(api.PoseRefineError) as e:
        api.select_greedy([0, 1], ov, 0, 0)
    assert "shared_den" in str(e.value)
    lib = _lib.load()
    od = np.arange(3, dtype=np.uint32)
    out = np.zeros(3, np.uint32)
    assert lib.pr_select_greedy(od.ctypes.data, 3, ov.ctypes.data, 6, 1, 4, out.ctypes.data, None) == _lib.PR_ERR_INVALID
    assert lib.pr_select_greedy(None, 3, ov.ctypes.data, 6, 1, 4, out.ctypes.data, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    assert lib.pr_select_greedy(od.ctypes.data, 3, None, 6, 1, 4, out.ctypes.data, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    assert lib.pr_select_greedy(od.ctypes.data, 3, ov.ctypes.data, 6, 1, 4, None, C.byref(C.c_uint32())) == _lib.PR_ERR_INVALID
    with pytest.raises(ValueError):
        api.select_greedy([0, 1], ov[:, :5], 1, 4)               # not square
    with pytest.raises(ValueError):
        api.select_greedy([0, -1], ov, 1, 4)


def _scores_for(ov, rng):
    P = len(ov)
    sc = np.zeros(P, api.SCORE)
    sc["inlier"] = np.diag(ov)
    sc["occluded"] = rng.integers(0, 50, P)
    sc["violation"] = rng.integers(0, 3000, P)
    sc["missing"] = rng.integers(0, 500, P)
    sc["visible"] = sc["inlier"] + sc["occluded"] + sc["violation"] + sc["missing"]
    return sc


@pytest.mark.parametrize("min_fraction", [0.0, 0.3, 0.5, 0.9, 1.0])
def test_select_hypotheses_uses_the_ranking_and_min_fraction(min_fraction):
    rng = np.random.default_rng(8)
    ov = _random_overlap(rng, 150)
    sc = _scores_for(ov, rng)
    frac = rank_fraction(sc)
    order = [int(i) for i in api.rank_hypotheses(sc) if frac[i] >= min_fraction]
    for ms in ((1, 4), (1, 2), (0, 1)):
        got = api.select_hypotheses(sc, ov, max_shared=ms, min_fraction=min_fraction)
        assert got.tolist() == greedy_ref(order, ov, *ms)
        assert (frac[got] >= min_fraction).all() and (np.diff(frac[got]) <= 0).all()        # best first
    assert api.select_hypotheses(sc, ov, min_fraction=min_fraction).tolist() == greedy_ref(order, ov, 1, 4)      # the default: a quarter
    # an explicit order replaces the ranking, min_fraction still applies
    rev = api.rank_hypotheses(sc)[::-1]
    want = greedy_ref([int(i) for i in rev if frac[i] >= min_fraction], ov, 1, 4)
    assert api.select_hypotheses(sc, ov, min_fraction=min_fraction, order=rev).tolist() == want


def test_select_hypotheses_empty_batch():
    assert api.select_hypotheses(np.zeros(0, api.SCORE), np.zeros((0, 0), np.uint32)).tolist() == []


def test_device_calls_without_gpu_fail_loudly():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    tri, pose, pj = np.zeros((1, 3, 3), np.float32), np.eye(4, dtype=np.float32)[None], np.eye(4, dtype=np.float32)
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap(tri, pose, 64, 48, pj, np.zeros((48, 64), np.int32), 5)
    assert e.value.code == _lib.PR_ERR_NO_DEVICE
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap_multi([tri], [0], pose, 64, 48, pj, np.zeros((48, 64), np.int32), 5)
    assert e.value.code == _lib.PR_ERR_NO_DEVICE
    lib = _lib.load()
    assert lib.pr_score_overlap(None, 0, None, 0, 64, 48, None, _lib.Roi(0, 0, 0, 0), None, 1, 5, None, None) == _lib.PR_ERR_NO_DEVICE
    assert lib.pr_score_overlap_multi(None, 0, None, None, 0, 64, 48, None, _lib.Roi(0, 0, 0, 0), None, 1, 5, None, None) == _lib.PR_ERR_NO_DEVICE
    # the selection itself needs no device
    assert api.select_greedy([1, 0], np.array([[5, 0], [0, 5]], np.uint32), 1, 4).tolist() == [1, 0]


def test_planted_frame_on_the_cpu(scenario):
    """Three instances of obj_06, 85 hypotheses around each (the exact pose first): exactly the three planted poses come back, best first,
    for every threshold -- from oracle renders, the numpy scores and the numpy matrix alone."""
    scene, poses = planted_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    assert poses.shape == (255, 4, 4) and PLANTED_EXACT == [0, 85, 170]
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    for tau in (5, 10):
        sc = score_ref(renders, scene, tau)
        ov = overlap_ref(renders, scene, tau)
        assert np.array_equal(ov, ov.T) and np.array_equal(np.diag(ov), sc["inlier"])
        for ms in ((1, 10), (1, 4), (1, 2)):
            for mf in (0.0, 0.5):
                got = api.select_hypotheses(sc, ov, max_shared=ms, min_fraction=mf)
                assert got.tolist() == PLANTED_SELECTION, (tau, ms, mf, got)
    # the pair kernel's ground is exercised, not skipped: most pairs share pixels
    assert np.count_nonzero(np.triu(ov, 1)) > 10000
