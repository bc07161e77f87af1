"""Mixed batches (hypotheses of several meshes in one call) without a GPU: the C ABI of the new entry points, the Python-side checks of
``mesh_index`` and the per-mesh ranking policy."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from pose_refine_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pr_render_multi", "pr_refine_batch_multi", "pr_score_poses_multi")


def test_header_declares_and_binding_binds_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "pose_refine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef struct \{ const pr_triangle \*tris_dev; size_t n_tris; \} pr_mesh_ref;", src)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
    assert C.sizeof(_lib.MeshRef) == 16
    assert _lib.load().pr_abi_version() == 4


def test_new_entry_points_report_no_device():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    lib = _lib.load()
    mesh = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0))
    idx = np.zeros(1, np.uint32)
    pose = np.eye(4, dtype=np.float32)
    proj = np.eye(4, dtype=np.float32)
    K = np.eye(3, dtype=np.float32)
    out = np.zeros(64 * 48, np.int32)
    assert lib.pr_render_multi(mesh, 1, idx.ctypes.data, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, _lib.Roi(0, 0, 0, 0),
                               out.ctypes.data) == _lib.PR_ERR_NO_DEVICE
    res = np.zeros(1, _lib.RESULT)
    sizes = np.zeros(1, np.uint32)
    scene = _lib.SceneProjDesc()
    assert lib.pr_refine_batch_multi(mesh, 1, idx.ctypes.data, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, K.ctypes.data, _lib.SCENE_PROJ,
                                     C.addressof(scene), _lib.Criteria(0, 0, 1), _lib.Roi(0, 0, 0, 0), res.ctypes.data,
                                     sizes.ctypes.data) == _lib.PR_ERR_NO_DEVICE
    sc = np.zeros(1, _lib.SCORE)
    assert lib.pr_score_poses_multi(mesh, 1, idx.ctypes.data, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, _lib.Roi(0, 0, 0, 0),
                                    out.ctypes.data, 1, 5, sc.ctypes.data) == _lib.PR_ERR_NO_DEVICE
    with pytest.raises(api.PoseRefineError) as e:
        api.refine_batch_multi([np.zeros((1, 3, 3), np.float32)], [0], pose[None], 64, 48, proj, K, api.Scene_projective())
    assert e.value.code == _lib.PR_ERR_NO_DEVICE


BAD_INDICES = [
    ("wrong length", lambda P: np.zeros(P - 1, np.int64)),
    ("too long", lambda P: np.zeros(P + 1, np.int64)),
    ("two-dimensional", lambda P: np.zeros((P, 1), np.int64)),
    ("negative", lambda P: np.array([0] * (P - 1) + [-1], np.int64)),
    ("equal to len(meshes)", lambda P: np.array([0] * (P - 1) + [2], np.int64)),
    ("far out of range", lambda P: np.array([1] * (P - 1) + [2**40], np.int64)),
    ("float", lambda P: np.zeros(P, np.float32)),
    ("bool", lambda P: np.zeros(P, bool)),
]


@pytest.mark.parametrize("what,make", BAD_INDICES, ids=[b[0] for b in BAD_INDICES])
def test_bad_mesh_index_raises_value_error_before_the_library(what, make, monkeypatch):
    # any library call would fail (no device here, or a poisoned loader): the check has to come first
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    P = 5
    meshes = [np.zeros((2, 3, 3), np.float32), np.zeros((1, 3, 3), np.float32)]
    poses = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    proj, K = np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)
    idx = make(P)
    with pytest.raises(ValueError):
        api.refine_batch_multi(meshes, idx, poses, 64, 48, proj, K, api.Scene_projective())
    with pytest.raises(ValueError):
        api.score_poses_multi(meshes, idx, poses, 64, 48, proj, np.zeros((48, 64), np.int32), 5)
    with pytest.raises(ValueError):
        api.render_multi(meshes, idx, poses, 64, 48, proj)


def _scores(rows):
    sc = np.zeros(len(rows), _lib.SCORE)
    for i, (vis, inl, occ) in enumerate(rows):
        sc[i]["visible"], sc[i]["inlier"], sc[i]["occluded"] = vis, inl, occ
    return sc


def test_rank_per_mesh_orders_within_each_mesh_with_original_indices():
    #            fraction     mesh
    rows = [(100, 50, 0),     # 0.50   0
            (10, 9, 0),       # 0.90   1
            (100, 90, 0),     # 0.90   0
            (0, 0, 0),        # empty  1
            (40, 20, 0),      # 0.50   0  -- tie with 0 in fraction, fewer inliers
            (20, 18, 0),      # 0.90   1  -- tie with 1 in fraction, more inliers
            (12, 6, 2),       # 0.60   3
            (30, 0, 30)]      # empty (only occluded)  3
    mesh_index = np.array([0, 1, 0, 1, 0, 1, 3, 3])
    sc = _scores(rows)
    got = api.rank_hypotheses_per_mesh(sc, mesh_index)
    assert sorted(got) == [0, 1, 3]                               # mesh 2 has no hypotheses: no entry
    assert got[0].tolist() == [2, 0, 4]
    assert got[1].tolist() == [5, 1, 3]
    assert got[3].tolist() == [6, 7]
    for m, order in got.items():                                  # the same policy as rank_hypotheses on the mesh's own scores
        members = np.flatnonzero(mesh_index == m)
        assert order.tolist() == members[api.rank_hypotheses(sc[members])].tolist()


def test_rank_per_mesh_exact_ties_keep_the_lower_index_first():
    sc = _scores([(10, 5, 0)] * 6)
    got = api.rank_hypotheses_per_mesh(sc, [2, 0, 2, 0, 2, 2])
    assert got[0].tolist() == [1, 3] and got[2].tolist() == [0, 2, 4, 5]


def test_rank_per_mesh_empty_batch_and_length_mismatch():
    assert api.rank_hypotheses_per_mesh(np.zeros(0, _lib.SCORE), np.zeros(0, np.int64)) == {}
    with pytest.raises(ValueError):
        api.rank_hypotheses_per_mesh(_scores([(1, 1, 0)] * 3), [0, 0])
