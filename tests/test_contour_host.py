"""Host side of the contour check (no GPU): the record layout, contour_fraction / filter_by_contour, the numpy reference (tests/contour_ref.py)
against a brute-force search and against the figures the definitions give on the scenario fixture, and the no-device error of the entry points."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from contour_ref import (NO_EDGE, contour_ref, distance_brute, distance_from_edges, edge_distance_ref, edges, jump_only, structured_scene)
from verify_ref import launch_split_case

W, H = synth.WIDTH, synth.HEIGHT


class PoseContour(C.Structure):
    """pr_pose_contour as the header declares it."""
    _fields_ = [("contour", C.c_uint32), ("hit", C.c_uint32), ("occluded", C.c_uint32), ("miss", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("dist_sum", C.c_uint64)]


def test_record_layout():
    assert C.sizeof(PoseContour) == 32 and api.CONTOUR.itemsize == 32 and _lib.CONTOUR is api.CONTOUR
    for name, _ in PoseContour._fields_:
        assert api.CONTOUR.fields[name][1] == getattr(PoseContour, name).offset, name
    assert api.CONTOUR.fields["dist_sum"][1] == 24 and api.CONTOUR.fields["reserved"][0].shape == (2,)
    assert api.CONTOUR_MAX_RADIUS == 32


def test_abi_version_is_unchanged():
    assert _lib.load().pr_abi_version() == 4


def _records(rows):
    out = np.zeros(len(rows), api.CONTOUR)
    for i, (c, h, o, m) in enumerate(rows):
        out[i]["contour"], out[i]["hit"], out[i]["occluded"], out[i]["miss"] = c, h, o, m
    return out


def test_contour_fraction_and_filter():
    rec = _records([(100, 50, 0, 50), (100, 50, 50, 0), (0, 0, 0, 0), (40, 0, 40, 0), (80, 20, 0, 60), (2**32 - 1, 2**31, 1, 2**31 - 2)])
    frac = api.contour_fraction(rec)
    assert frac.dtype == np.float64
    assert frac.tolist() == [0.5, 1.0, 0.0, 0.0, 0.25, 2**31 / (2**32 - 2)]
    order = np.array([4, 1, 0, 5, 3, 2])
    assert api.filter_by_contour(order, rec, 0.5).tolist() == [1, 0, 5]
    assert api.filter_by_contour(order, rec, 0.0).tolist() == order.tolist()
    assert api.filter_by_contour(order, rec, 0.26).dtype == np.int64
    assert api.filter_by_contour(order[:2], rec, 0.3).tolist() == [1]              # a partial order stays partial
    assert api.filter_by_contour(np.zeros(0, np.int64), rec, 0.3).tolist() == []
    assert api.filter_by_contour(order, rec, 1.5).tolist() == []


def test_filter_feeds_select_hypotheses():
    scores = np.zeros(3, api.SCORE)
    scores["visible"], scores["inlier"] = [100, 100, 100], [90, 80, 70]
    overlap = np.diag(scores["inlier"]).astype(np.uint32)
    rec = _records([(50, 5, 0, 45), (50, 40, 0, 10), (50, 45, 0, 5)])
    order = api.filter_by_contour(api.rank_hypotheses(scores), rec, 0.5)
    assert order.tolist() == [1, 2]                              # the best-ranked hypothesis has no contour support
    assert api.select_hypotheses(scores, overlap, order=order).tolist() == [1, 2]


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (33, 1), (23, 31), (40, 70)])
@pytest.mark.parametrize("radius", [0, 1, 3, 32])
def test_reference_distance_against_brute_force(shape, radius):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + radius)
    for density in (0.0, 0.002, 0.03, 0.5):
        e = rng.random(shape) < density
        D = distance_from_edges(e, radius)
        assert D.dtype == np.uint8 and np.array_equal(D, distance_brute(e, radius)), (shape, radius, density)
        assert ((D == 0) == e).all()
        if not e.any():
            assert (D == NO_EDGE).all()


def test_reference_edges_by_hand():
    d = np.array([[0, 0, 0, 0, 0],
                  [0, 100, 100, 100, 0],
                  [0, 100, 100, 100, 130],
                  [0, 100, 100, 111, 130]], np.int32)
    want = np.array([[0, 0, 0, 0, 0],
                     [0, 1, 1, 1, 0],
                     [0, 1, 0, 1, 1],
                     [0, 1, 1, 1, 0]], bool)                     # the nearer side only; the frame border ends no surface ((3, 4) has none)
    assert np.array_equal(edges(d, 10), want)
    assert edges(d, 10)[3, 2] and not edges(d, 11)[3, 2]         # 111 - 100 = 11 must EXCEED the jump
    assert edges(d, 18)[3, 3] and not edges(d, 19)[3, 3]
    assert edges(d, 29)[2, 3] and not edges(d, 30)[2, 3]
    assert np.argwhere(jump_only(d, 10)).tolist() == [[2, 3]]    # the one edge pixel whose four neighbours all hold a depth
    ext = np.array([[2**31 - 1, 1, -2**31, 5]], np.int32)        # differences need 64 bits
    assert edges(ext, 0).tolist() == [[False, True, False, True]]
    assert edges(ext, 2**31 - 1).tolist() == [[False, True, False, True]]
    assert edges(np.array([[1, 2**31 - 1]], np.int32), 2**31 - 3).tolist() == [[True, False]]
    assert edges(np.array([[1, 2**31 - 1]], np.int32), 2**31 - 2).tolist() == [[False, False]]


def test_reference_figures_on_the_scenario(scenario):
    """The definitions on obj_06 at the scene pose: edge counts per jump, the scene pose against its own render, and hits falling as the pose
    is pushed sideways (radius 3, jump 10, tau 5)."""
    d1 = scenario["depth"][1]
    assert [int(edges(d1, j).sum()) for j in (5, 10, 20)] == [866, 823, 748]
    D = edge_distance_ref(d1, 10, 3)
    own = contour_ref(scenario["depth"][1:2], d1, 5, 10, D)[0]
    assert (own["contour"], own["hit"], own["occluded"], own["miss"], own["dist_sum"]) == (823, 823, 0, 0, 0)
    hits, misses = [], []
    for shift in (2, 5, 10, 20):
        p = scenario["poses"][1].copy()
        p[0, 3] += shift
        c = contour_ref(O.render(scenario["tris"], p[None], W, H, scenario["proj"]), d1, 5, 10, D)[0]
        assert 815 <= c["contour"] <= 835
        hits.append(int(c["hit"]))
        misses.append(int(c["miss"]))
    assert hits == [672, 320, 196, 142] and misses == [21, 273, 368, 446]


def test_structured_scene_has_every_class(scenario):
    sc = structured_scene(scenario["depth"][1])
    assert sc.dtype == np.int32 and sc.min() >= 0 and sc.max() < 2**16
    n_edges = int(edges(sc, 10).sum())
    assert 1000 < n_edges < sc.size // 20                        # structure, not salt noise
    poses = synth.hypotheses(16)
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    c = contour_ref(r, sc, 5, 10, edge_distance_ref(sc, 10, 2))
    for f in ("hit", "occluded", "miss", "dist_sum"):
        assert (c[f] > 0).all(), f
    assert jump_only(r, 10).sum() > 0


def test_launch_split_case_is_pinned():
    """The inputs of the GPU tests of a batch that needs two launches over its boxes: what the references hold for the 8 distinct poses."""
    c = launch_split_case()
    assert (c["W"], c["H"], c["P"]) == (48, 32, 32768 + 5) and c["tris"].shape == (12, 3, 3) and c["poses"].shape == (8, 4, 4)
    assert len({p.tobytes() for p in c["poses"]}) == 8
    assert c["scene"].dtype == np.int32 and c["scene"].shape == (32, 48) and 0 <= c["scene"].min() and c["scene"].max() < 2**16
    sc, con = c["scores"], c["contours"]
    assert (sc["visible"] > 0).all() and np.count_nonzero((sc["inlier"] > 0) & (con["contour"] > 0)) >= 4
    assert sc["visible"].tolist() == [301, 394, 272, 176, 172, 123, 161, 670]
    assert sc["inlier"].tolist() == [107, 252, 109, 51, 103, 0, 6, 0]
    assert sc["abs_err_sum"].tolist() == [243, 546, 261, 109, 209, 0, 14, 0]
    assert con["contour"].tolist() == [123, 84, 81, 40, 94, 38, 81, 75] and con["hit"].tolist() == [39, 66, 48, 15, 75, 15, 69, 69]
    rows = [np.flatnonzero((r > 0).any(1)) for r in c["renders"]]
    assert sum(ys[0] < 16 <= ys[-1] for ys in rows) >= 4              # boxes that lie in both row blocks
    drawn = (c["renders"] > 0).any(0)
    assert drawn[0].any() and drawn[-1].any() and drawn[:, 0].any() and drawn[:, -1].any()


def test_device_calls_without_gpu_fail_loudly():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    lib = _lib.load()
    assert lib.pr_scene_edge_distance_dev(None, 1, 64, 48, 10, 3, None) == _lib.PR_ERR_NO_DEVICE
    assert lib.pr_score_contours(None, 0, None, 0, 64, 48, None, _lib.Roi(0, 0, 0, 0), None, 1, 5, 10, None, None, None, None) == _lib.PR_ERR_NO_DEVICE
    assert lib.pr_score_contours_multi(None, 0, None, None, 0, 64, 48, None, _lib.Roi(0, 0, 0, 0), None, 1, 5, 10, None, None, None,
                                       None) == _lib.PR_ERR_NO_DEVICE
    with pytest.raises(api.PoseRefineError) as e:
        api.scene_edge_distance(np.zeros((48, 64), np.int32), 64, 48, 10, 3)
    assert e.value.code == _lib.PR_ERR_NO_DEVICE
