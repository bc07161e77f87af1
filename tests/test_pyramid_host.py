"""Coarse-to-fine refinement (pr_refine_pyramid) without a GPU: the composed reference against the oracle's own batch, the C ABI of the new
entry points and their level-table checks, and the quality of the default schedule on the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pyramid_ref as R
from pose_refine_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = synth.WIDTH, synth.HEIGHT
NEW = ("pr_refine_pyramid", "pr_refine_pyramid_multi")


@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_reference_with_one_full_level_is_the_oracles_batch(scenario, kind):
    """The yardstick itself: one level of stride 1 composed from render / depth2cloud / icp equals po_refine_batch byte for byte,
    full frame and with an ROI that cuts the object."""
    poses = synth.hypotheses(4)
    crit = (0.0, 0.0, 6)
    scene = scenario["proj_scene" if kind == "proj" else "nn_scene"]
    for roi in ((0, 0, 0, 0), (161, 81, 320, 240)):
        res, lres, lsizes = R.refine_pyramid(scenario["tris"], poses, W, H, scenario["proj"], scenario["K"], scene, [(1, crit)], 2048, roi)
        ores, osizes, _ = O.refine_batch(scenario["tris"], poses, W, H, scenario["proj"], scenario["K"], scene, crit, O.SUM_CANONICAL, 2048, roi)
        assert np.array_equal(lsizes[0], osizes) and osizes.min() > 0
        assert res.tobytes() == ores.tobytes() and lres[0].tobytes() == ores.tobytes()


def test_header_declares_and_binding_binds_the_pyramid_entry_points():
    src = open(os.path.join(ROOT, "include", "pose_refine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef struct \{ uint32_t stride; pr_criteria crit; \} pr_pyramid_level;", src)
    assert re.search(r"#define PR_PYRAMID_MAX_LEVELS 4\b", src) and re.search(r"#define PR_PYRAMID_MAX_STRIDE 16\b", src)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
    assert C.sizeof(_lib.PyramidLevel) == 16
    assert (_lib.PYRAMID_MAX_LEVELS, _lib.PYRAMID_MAX_STRIDE) == (4, 16)
    lv = api.PyramidLevel(3, api.ICPConvergenceCriteria(1e-5, 2e-5, 7))
    assert isinstance(lv, _lib.PyramidLevel) and lv.stride == 3 and lv.crit.max_iteration == 7
    assert R.plain_levels([lv]) == R.plain_levels([(3, (np.float32(1e-5), np.float32(2e-5), 7))])
    assert api.PYRAMID_DEFAULT == ((4, (0, 0, 12)), (2, (0, 0, 5)), (1, (0, 0, 3)))
    assert 1 <= len(api.PYRAMID_DEFAULT) <= _lib.PYRAMID_MAX_LEVELS
    assert _lib.load().pr_abi_version() == 4                      # no existing structure changed


def _bare_scene():
    """A projective scene whose arrays are empty device vectors (nothing is allocated): enough for the argument checks."""
    sc = api.Scene_projective()
    sc.pcd_buffer = sc.normal_buffer = api.DeviceVector(0)
    return sc


BAD_TABLES = [
    ("no level", []),
    ("five levels", [(1, (0, 0, 1))] * 5),
    ("stride 0", [(4, (0, 0, 2)), (0, (0, 0, 2))]),
    ("stride 17", [(17, (0, 0, 2)), (1, (0, 0, 2))]),
    ("negative max_iteration", [(2, (0, 0, 2)), (1, (0, 0, -1))]),
]


@pytest.mark.parametrize("what,levels", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_level_table_is_invalid_before_any_device_is_touched(what, levels):
    """PR_ERR_INVALID with the outputs untouched -- the same on a box without a GPU, where everything else reports PR_ERR_NO_DEVICE."""
    pose = np.eye(4, dtype=np.float32)[None]
    proj, K = np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)
    with pytest.raises(api.PoseRefineError) as e:
        api.refine_pyramid(api.DeviceVector(0), pose, 64, 48, proj, K, _bare_scene(), levels)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_refine_pyramid" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:
        api.refine_pyramid_multi([api.DeviceVector(0)], [0], pose, 64, 48, proj, K, _bare_scene(), levels)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_refine_pyramid_multi" in str(e.value)
    # the C ABI directly: nothing is written
    lib = _lib.load()
    table = (_lib.PyramidLevel * max(1, len(levels)))(*[api.PyramidLevel(*lv) for lv in levels])
    res = np.full(1, 7, np.uint8).repeat(72).view(_lib.RESULT)
    lres = np.full(5 * 72, 7, np.uint8)
    lsz = np.full(5, 0x07070707, np.uint32)
    scene = _lib.SceneProjDesc()
    rc = lib.pr_refine_pyramid(None, 0, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, K.ctypes.data, _lib.SCENE_PROJ, C.addressof(scene),
                               table, len(levels), _lib.Roi(0, 0, 0, 0), res.ctypes.data, lres.ctypes.data, lsz.ctypes.data)
    assert rc == _lib.PR_ERR_INVALID
    assert (res.view(np.uint8) == 7).all() and (lres == 7).all() and (lsz == 0x07070707).all()


def test_null_table_or_null_results_are_invalid():
    lib = _lib.load()
    pose = np.eye(4, dtype=np.float32)[None]
    proj, K = np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)
    scene = _lib.SceneProjDesc()
    table = (_lib.PyramidLevel * 1)(api.PyramidLevel(1, (0, 0, 1)))
    res = np.zeros(1, _lib.RESULT)
    mesh = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0))
    idx = np.zeros(1, np.uint32)
    for levels, out in ((None, res.ctypes.data), (table, None)):
        assert lib.pr_refine_pyramid(None, 0, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, K.ctypes.data, _lib.SCENE_PROJ, C.addressof(scene),
                                     levels, 1, _lib.Roi(0, 0, 0, 0), out, None, None) == _lib.PR_ERR_INVALID
        assert lib.pr_refine_pyramid_multi(mesh, 1, idx.ctypes.data, pose.ctypes.data, 1, 64, 48, proj.ctypes.data, K.ctypes.data, _lib.SCENE_PROJ,
                                           C.addressof(scene), levels, 1, _lib.Roi(0, 0, 0, 0), out, None, None) == _lib.PR_ERR_INVALID


def test_good_level_table_reports_no_device():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    pose = np.eye(4, dtype=np.float32)[None]
    proj, K = np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)
    for levels in (api.PYRAMID_DEFAULT, [(16, (1e-5, 1e-5, 0))], [api.PyramidLevel(1, api.ICPConvergenceCriteria())] * 4):
        with pytest.raises(api.PoseRefineError) as e:
            api.refine_pyramid(api.DeviceVector(0), pose, 64, 48, proj, K, _bare_scene(), levels)
        assert e.value.code == _lib.PR_ERR_NO_DEVICE
        with pytest.raises(api.PoseRefineError) as e:
            api.refine_pyramid_multi([api.DeviceVector(0)], [0], pose, 64, 48, proj, K, _bare_scene(), levels)
        assert e.value.code == _lib.PR_ERR_NO_DEVICE


def test_default_schedule_reaches_the_full_resolution_optimum_on_the_oracle(scenario):
    """api.PYRAMID_DEFAULT against 20 full-resolution iterations, oracle only (canonical sums, 2048 points per block), synth.hypotheses(48),
    projective scene.  Among the hypotheses the full run converges on (fitness >= 0.9) the final translations differ by at most 0.05 mm --
    three times the 0.016 mm measured when the schedule was chosen; the margin is for another schedule's rounding path -- and at least 40 of
    the 48 qualify (the full run alone gives 43)."""
    poses = synth.hypotheses(48)
    scene = scenario["proj_scene"]
    full, _, _ = O.refine_batch(scenario["tris"], poses, W, H, scenario["proj"], scenario["K"], scene, (0.0, 0.0, 20), O.SUM_CANONICAL, 2048)
    res, lres, lsizes = R.refine_pyramid(scenario["tris"], poses, W, H, scenario["proj"], scenario["K"], scene, api.PYRAMID_DEFAULT, 2048)
    ok = full["fitness"] >= 0.9
    dt = np.linalg.norm((res["T"].reshape(-1, 4, 4)[:, :3, 3].astype(np.float64) - full["T"].reshape(-1, 4, 4)[:, :3, 3].astype(np.float64)), axis=1) * 1000.0
    work = float((lsizes.astype(np.float64) * np.array([[lv[1][2] + 1] for lv in api.PYRAMID_DEFAULT])).sum() / (lsizes[-1].astype(np.float64) * 21).sum())
    print(f"converged {int(ok.sum())} of 48; max |dt| {dt[ok].max():.4f} mm; point-passes {work:.3f} of the full run's")
    assert int(ok.sum()) >= 40
    assert dt[ok].max() <= 0.05
