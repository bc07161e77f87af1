"""Host side of render-and-compare verification (no GPU): the pr_pose_score layout, pr_refined_poses and the ranking policy."""
import ctypes as C

import numpy as np
import pytest

from pose_refine_amd import _lib, api, synth


class PoseScore(C.Structure):          # pr_pose_score as the header declares it
    _fields_ = [("visible", C.c_uint32), ("inlier", C.c_uint32), ("occluded", C.c_uint32), ("violation", C.c_uint32),
                ("missing", C.c_uint32), ("reserved", C.c_uint32), ("abs_err_sum", C.c_uint64)]


def test_score_record_layout():
    assert C.sizeof(PoseScore) == 32 and api.SCORE.itemsize == 32
    for name, _ in PoseScore._fields_:
        assert getattr(PoseScore, name).offset == api.SCORE.fields[name][1], name
    assert [api.SCORE.fields[f][1] for f in ("visible", "inlier", "occluded", "violation", "missing", "reserved", "abs_err_sum")] == [0, 4, 8, 12, 16, 20, 24]


def _results(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, api.RESULT)
    for i in range(n):
        a = rng.normal(size=3) * 0.02
        c, s = np.cos(a), np.sin(a)
        Rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
        Ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
        Rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
        T = np.eye(4)
        T[:3, :3] = Rz @ Ry @ Rx
        T[:3, 3] = rng.normal(size=3) * 0.01                       # metres
        rec["T"][i] = T.astype(np.float32).reshape(-1)
    rec["fitness"] = 0.9
    return rec


def test_refined_poses_is_the_documented_product():
    poses = synth.hypotheses(8)
    rec = _results(8)
    got = api.refined_poses(rec, poses)
    lib = _lib.load()
    for i in range(8):
        Tp = rec["T"][i].copy()
        Tp[[3, 7, 11]] *= np.float32(1000.0)
        want = np.zeros(16, np.float32)
        lib.pr_mat4_mul(Tp.ctypes.data, np.ascontiguousarray(poses[i], np.float32).ctypes.data, want.ctypes.data)
        assert np.array_equal(got[i].reshape(-1), want), i
        f64 = Tp.astype(np.float64).reshape(4, 4) @ poses[i].astype(np.float64)
        assert np.allclose(got[i], f64, rtol=0, atol=1e-4), i
    # the identity result leaves the pose as it is
    ident = np.zeros(1, api.RESULT)
    ident["T"][0] = np.eye(4, dtype=np.float32).reshape(-1)
    assert np.array_equal(api.refined_poses(ident, poses[:1])[0], poses[0])
    with pytest.raises(ValueError):
        api.refined_poses(rec[:3], poses)


def _scores(rows):
    out = np.zeros(len(rows), api.SCORE)
    for i, (vis, inl, occ, vio, mis) in enumerate(rows):
        out[i] = (vis, inl, occ, vio, mis, 0, 0)
    return out


def test_rank_hypotheses_policy():
    sc = _scores([
        (100, 50, 0, 50, 0),       # 0: 0.5
        (0, 0, 0, 0, 0),           # 1: nothing rendered -> last
        (100, 80, 20, 0, 0),       # 2: 80 / 80 = 1.0
        (10, 10, 0, 0, 0),         # 3: 1.0, fewer inliers than 2
        (200, 100, 0, 0, 100),     # 4: 0.5, more inliers than 0
        (100, 50, 0, 0, 50),       # 5: 0.5, same inliers as 0 -> after 0 (lower index first)
        (30, 0, 30, 0, 0),         # 6: only occluded pixels -> last, after 1
        (100, 80, 20, 0, 0),       # 7: same as 2 -> after 2
    ])
    assert api.rank_hypotheses(sc).tolist() == [2, 7, 3, 4, 0, 5, 1, 6]
    assert api.rank_hypotheses(sc).dtype == np.int64
    assert api.rank_hypotheses(np.zeros(0, api.SCORE)).tolist() == []
    # large counts: the fraction is evaluated in float64 (in float32, 4294967294 / 4294967295 rounds to 1.0 and the tie-break would put 0 first)
    big = _scores([(4294967295, 4294967294, 0, 1, 0), (1000, 1000, 0, 0, 0)])
    assert api.rank_hypotheses(big).tolist() == [1, 0]


def test_score_poses_without_gpu_fails_loudly():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    with pytest.raises(api.PoseRefineError) as e:
        api.score_poses(np.zeros((1, 3, 3), np.float32), np.eye(4, dtype=np.float32)[None], 64, 48, np.eye(4, dtype=np.float32),
                        np.zeros((48, 64), np.int32), 5)
    assert e.value.code == _lib.PR_ERR_NO_DEVICE
    # the C entry point itself (no upload in front of it)
    rc = _lib.load().pr_score_poses(None, 0, None, 0, 64, 48, None, _lib.Roi(0, 0, 0, 0), None, 1, 5, None)
    assert rc == _lib.PR_ERR_NO_DEVICE
