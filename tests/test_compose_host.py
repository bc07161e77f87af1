"""Host side of the composition (no GPU): the two symbols and their records, visible_fraction, the no-device error, and the numpy reference
(tests/compose_ref.py) on hand-made renders and on the planted frame of the selection tests."""
import ctypes as C
import os

import numpy as np

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from compose_ref import check_invariants, compose_ref
from select_ref import PLANTED_EXACT, planted_frame
from verify_ref import score_ref

W, H = synth.WIDTH, synth.HEIGHT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PoseVisible(C.Structure):
    """pr_pose_visible as the header declares it."""
    _fields_ = [("owned", C.c_uint32), ("owned_inlier", C.c_uint32), ("owned_occluded", C.c_uint32), ("owned_violation", C.c_uint32),
                ("owned_missing", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class FrameExplained(C.Structure):
    """pr_frame_explained as the header declares it."""
    _fields_ = [("window", C.c_uint32), ("measured", C.c_uint32), ("covered", C.c_uint32), ("explained", C.c_uint32), ("in_front", C.c_uint32),
                ("behind", C.c_uint32), ("unmeasured", C.c_uint32), ("reserved", C.c_uint32)]


def test_symbols_and_record_layouts():
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in ("pr_compose_detections", "pr_compose_detections_multi"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert len(_lib.SIGNATURES["pr_compose_detections"][1]) == 16 and len(_lib.SIGNATURES["pr_compose_detections_multi"][1]) == 17
    assert C.sizeof(PoseVisible) == 32 == api.VISIBLE.itemsize and C.sizeof(FrameExplained) == 32 == api.FRAME.itemsize
    for dt, st in ((api.VISIBLE, PoseVisible), (api.FRAME, FrameExplained)):
        for name, _ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    assert lib.pr_abi_version() == 4                              # no existing struct changed
    assert api.COMPOSE_NONE == 0xFFFF and api.COMPOSE_MAX_POSES == 65535
    header = open(os.path.join(ROOT, "include", "pose_refine.h")).read()
    assert "#define PR_COMPOSE_NONE      0xFFFFu" in header and "#define PR_COMPOSE_MAX_POSES 65535u" in header


def test_visible_fraction():
    sc = np.zeros(5, api.SCORE)
    vi = np.zeros(5, api.VISIBLE)
    sc["visible"] = [100, 80, 0, 7, 4000000000]
    vi["owned"] = [100, 20, 0, 0, 1000000000]
    frac = api.visible_fraction(sc, vi)
    assert frac.dtype == np.float64 and frac.tolist() == [1.0, 0.25, 0.0, 0.0, 0.25]
    assert api.visible_fraction(np.zeros(0, api.SCORE), np.zeros(0, api.VISIBLE)).shape == (0,)


def test_too_many_poses_is_refused_before_any_device_use():
    """The limit is checked first: the same answer with and without a GPU, with nothing read or written."""
    lib = _lib.load()
    roi = _lib.Roi(0, 0, 0, 0)
    assert lib.pr_compose_detections(None, 0, None, 65536, 64, 48, None, roi, None, 1, 5, None, None, None, None, None) == _lib.PR_ERR_INVALID
    msg = lib.pr_last_error().decode()
    assert "PR_COMPOSE_MAX_POSES" in msg and "65535" in msg and "65536" in msg and "pr_compose_detections" in msg
    assert lib.pr_compose_detections_multi(None, 0, None, None, 65536, 64, 48, None, roi, None, 1, 5, None, None, None, None, None) == _lib.PR_ERR_INVALID
    assert "PR_COMPOSE_MAX_POSES" in lib.pr_last_error().decode() and "pr_compose_detections_multi" in lib.pr_last_error().decode()


def test_device_calls_need_a_device():
    """Without a GPU every call fails with PR_ERR_NO_DEVICE; with one, a call without hypotheses is PR_OK and writes nothing."""
    want = _lib.PR_OK if api.device_count() > 0 else _lib.PR_ERR_NO_DEVICE
    lib = _lib.load()
    pj = np.eye(4, dtype=np.float32)
    roi = _lib.Roi(0, 0, 0, 0)
    assert lib.pr_compose_detections(None, 0, None, 0, 64, 48, pj.ctypes.data, roi, None, 1, 5, None, None, None, None, None) == want
    assert lib.pr_compose_detections_multi(None, 0, None, None, 0, 64, 48, pj.ctypes.data, roi, None, 1, 5, None, None, None, None, None) == want
    if want != _lib.PR_OK:
        tri, pose = np.zeros((1, 3, 3), np.float32), np.eye(4, dtype=np.float32)[None]
        for call in (lambda: api.compose_detections(tri, pose, 64, 48, pj, np.zeros((48, 64), np.int32), 5),
                     lambda: api.compose_detections_multi([tri], [0], pose, 64, 48, pj, np.zeros((48, 64), np.int32), 5)):
            try:
                call()
            except api.PoseRefineError as e:
                assert e.code == _lib.PR_ERR_NO_DEVICE
            else:
                raise AssertionError("a device call succeeded without a device")


def test_reference_on_hand_made_renders():
    """Ties go to the lower index, duplicates own nothing, the ROI window is placed in the frame, and the four classes are pr_pose_score's."""
    r = np.zeros((4, 2, 3), np.int32)
    r[0] = [[500, 500, 0], [0, 700, 0]]
    r[1] = [[500, 400, 0], [0, 700, 900]]
    r[2] = r[0]
    r[3] = [[0, 0, 0], [0, 0, 0]]
    scene = np.array([[0, 0, 0, 0, 0], [0, 503, 380, 0, 0], [0, 0, 700, 0, 0], [0, 0, 0, 0, 0]], np.int32)
    c = compose_ref(r, scene, 3, roi=(1, 1, 3, 2))
    assert c.labels.tolist() == [[0xFFFF] * 5, [0xFFFF, 0, 1, 0xFFFF, 0xFFFF], [0xFFFF, 0xFFFF, 0, 1, 0xFFFF], [0xFFFF] * 5]
    assert c.depth.tolist() == [[0] * 5, [0, 500, 400, 0, 0], [0, 0, 700, 900, 0], [0] * 5]
    assert c.ties.tolist() == [[0] * 5, [0, 3, 1, 0, 0], [0, 0, 3, 1, 0], [0] * 5]
    assert c.visible["owned"].tolist() == [2, 2, 0, 0] and c.visible["owned_inlier"].tolist() == [2, 0, 0, 0]
    assert c.visible["owned_occluded"].tolist() == [0, 1, 0, 0] and c.visible["owned_missing"].tolist() == [0, 1, 0, 0]
    f = c.frame
    assert (f["window"], f["measured"], f["covered"], f["explained"], f["in_front"], f["behind"], f["unmeasured"]) == (6, 3, 4, 2, 0, 1, 1)
    check_invariants(c, score_ref(r, scene, 3, (1, 1, 3, 2)))
    # the composite in front of the measurement: `violation` of the owner, `in_front` of the frame
    c = compose_ref(r[1:2], np.full((2, 3), 1000, np.uint16), 3)
    assert c.visible["owned_violation"].tolist() == [4] and c.frame["in_front"] == 4 and c.frame["measured"] == 6
    # a generator of renders, and no renders at all
    c = compose_ref((x for x in r), scene, 3, roi=(1, 1, 3, 2))
    assert c.visible["owned"].tolist() == [2, 2, 0, 0]
    c = compose_ref(np.zeros((0, 2, 3), np.int32), scene[:2, :3], 3)
    assert len(c.visible) == 0 and c.frame["covered"] == 0 and (c.labels == 0xFFFF).all()


def test_planted_frame_on_the_cpu(scenario):
    """The three planted instances composed in the order [0, 85, 170]: instance 0 stands 60 mm behind instance 1 and loses the pixels they share."""
    scene, poses = planted_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    renders = O.render(scenario["tris"], poses[PLANTED_EXACT], W, H, scenario["proj"])
    sc = score_ref(renders, scene, 5)
    c = compose_ref(renders, scene, 5)
    check_invariants(c, sc)
    assert sc["visible"].tolist() == [15538, 21960, 11965]
    assert c.visible["owned"].tolist() == [11975, 21936, 11965]
    assert int(sc["visible"][0]) - int(c.visible["owned"][0]) == 3563
    assert api.visible_fraction(sc, c.visible).tolist() == [11975 / 15538, 21936 / 21960, 1.0]
    assert c.frame["window"] == W * H and c.frame["covered"] == 11975 + 21936 + 11965
    assert int(c.frame["explained"]) * 10 > int(c.frame["covered"]) * 8      # the planted poses explain the frame they were planted in
    # the order of the poses decides ties only: the same pixels, the same depth
    rev = compose_ref(renders[::-1], scene, 5)
    assert np.array_equal(rev.depth, c.depth) and rev.frame.tobytes() == c.frame.tobytes()
    same = rev.labels == np.where(c.labels == api.COMPOSE_NONE, api.COMPOSE_NONE, 2 - c.labels.astype(np.int64))
    assert np.array_equal(~same, c.ties > 1)
