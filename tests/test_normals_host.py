"""Host side of the normal agreement (no GPU): the numpy reference (tests/normals_ref.py) against the true normal of tilted planes and against
the figures the definition gives on the scenario fixture, the record layout, normal_fraction / filter_by_normals, and the argument checks
that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from pose_refine_amd import _lib, api, synth
from normals_ref import agreement, assert_identities, normal_of, normals_ref
from verify_ref import score_ref

W, H = synth.WIDTH, synth.HEIGHT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS30 = float(np.cos(np.deg2rad(30.0)))
STEP, JUMP = 4, 20


class PoseNormal(C.Structure):
    """pr_pose_normal as the header declares it."""
    _fields_ = [("tested", C.c_uint32), ("agree", C.c_uint32), ("disagree", C.c_uint32), ("no_render_normal", C.c_uint32),
                ("no_scene_normal", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def test_abi_and_record_layout():
    assert _lib.load().pr_abi_version() == 4
    assert C.sizeof(PoseNormal) == 32 and api.NORMAL.itemsize == 32 and _lib.NORMAL is api.NORMAL
    for name, _ in PoseNormal._fields_:
        assert api.NORMAL.fields[name][1] == getattr(PoseNormal, name).offset, name
    assert api.NORMAL.fields["reserved"][0].shape == (3,)
    assert api.NORMAL_MAX_STEP == 8
    header = open(os.path.join(ROOT, "include", "pose_refine.h")).read()
    assert "#define PR_NORMAL_MAX_STEP 8" in header and "#define PR_ABI_VERSION 4" in header


# ---- the estimator against the truth ------------------------------------------------------------------------------------------------------
def _plane_depth(w, h, K, tilt_deg, z0=1.0e6):
    """rint of the depth of the plane through (0, 0, z0) whose normal is (0, 0, 1) turned by tilt_deg about the axis (0.6, 0.8, 0), and that normal."""
    ax = np.array([0.6, 0.8, 0.0])
    t = np.deg2rad(tilt_deg)
    kx = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    n = (np.eye(3) + np.sin(t) * kx + (1.0 - np.cos(t)) * (kx @ kx)) @ np.array([0.0, 0.0, 1.0])
    k = np.asarray(K, np.float64)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.stack([(x - k[2]) / k[0], (y - k[5]) / k[4], np.ones_like(x)], -1)
    return np.rint(n[2] * z0 / (ray @ n)).astype(np.int64), n


@pytest.mark.parametrize("step", [1, 2, 4, 8])
@pytest.mark.parametrize("tilt", [0.0, 20.0, 40.0])
def test_plane_truth(tilt, step):
    """Measured with this reference: exactly 0 at tilt 0; 0.084 degrees at tilt 40, step 8, the worst case; at most 0.024 degrees elsewhere.  The bound of 0.2 degrees covers the second-order error of a central difference under perspective, nothing else."""
    w, h = 160, 120
    K = (synth.K_TEST / np.float32(4.0)).astype(np.float32)
    d, n = _plane_depth(w, h, K, tilt)
    assert d.min() > 4.0e5                                         # so far away that the rounding to integers plays no part
    defined, a, b, c = normal_of(d, K, step, 2**40)
    inner = np.zeros((h, w), bool)
    inner[step:h - step, step:w - step] = True
    assert np.array_equal(defined, inner)                          # defined exactly where the four neighbours lie inside the image
    a, b, c = a[defined], b[defined], c[defined]
    assert (c > 0).all()                                           # away from the camera
    if tilt == 0.0:
        assert (a == 0).all() and (b == 0).all()                   # exact for a fronto-parallel plane
    cosang = (a * n[0] + b * n[1] + c * n[2]) / np.sqrt(a * a + b * b + c * c)
    err = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).max()
    print(f"tilt {tilt} step {step}: worst angle to the true normal {err:.4f} degrees")
    assert err <= 0.2
    if tilt == 0.0:
        assert err == 0.0


# ---- the records on the scenario -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hyps16():
    return synth.hypotheses(16, seed=6)


@pytest.fixture(scope="module")
def renders16(scenario, hyps16):
    import oracle_lib as O
    return O.render(scenario["tris"], hyps16, W, H, scenario["proj"])


def test_identities(scenario, renders16):
    scene = scenario["depth"][1]
    for tau, step, jump, cos_min in ((5, STEP, JUMP, COS30), (20, 1, 3, 0.0), (8, 8, 50, 1.0)):
        rec = normals_ref(renders16, scene, tau, scenario["K"], step, jump, cos_min)
        assert_identities(rec, score_ref(renders16, scene, tau))
        assert rec["tested"].sum() > 0 and rec["no_render_normal"].sum() > 0
    frac = api.normal_fraction(normals_ref(renders16, scene, 5, scenario["K"], STEP, JUMP, COS30))
    assert 0.0 <= frac.min() and frac.max() <= 1.0


def test_self_agreement(scenario, renders16):
    for i in (0, 3, 7):
        img = renders16[i]
        for cos_min in (COS30, 1.0):
            rec = normals_ref(img[None], img, 0, scenario["K"], STEP, JUMP, cos_min)[0]
            assert rec["tested"] > 1000 and rec["agree"] == rec["tested"] and rec["disagree"] == 0 and rec["no_scene_normal"] == 0
            assert rec["tested"] + rec["no_render_normal"] == np.count_nonzero(img)


def test_the_cue_works(scenario):
    """obj_06 at the model pose against a flat wall at 300 mm with a wide tau: every rendered pixel is a depth inlier, and the normals say no."""
    img = scenario["depth"][0]
    wall = np.full((H, W), 300, np.int32)
    sc = score_ref(img[None], wall, 60)[0]
    assert sc["inlier"] == sc["visible"] == np.count_nonzero(img) > 20000
    on_wall = normals_ref(img[None], wall, 60, scenario["K"], STEP, JUMP, COS30)
    on_itself = normals_ref(img[None], img, 60, scenario["K"], STEP, JUMP, COS30)
    rec = np.concatenate([on_wall, on_itself])
    frac = api.normal_fraction(rec)
    print(f"normal_fraction on the wall {frac[0]:.4f} ({rec[0]}), on itself {frac[1]:.4f}")
    assert frac[0] < 0.5 and frac[1] == 1.0
    assert rec["tested"][0] == rec["tested"][1] > 20000            # a wall has a normal everywhere the render has one
    assert api.filter_by_normals(np.array([0, 1]), rec, 0.5).tolist() == [1]


def test_noise_and_step(scenario):
    """+-1 mm of noise on millimetre depth: a 1-pixel difference is useless, a wider one is not -- which is why the step is a parameter."""
    img = scenario["depth"][1]
    rng = np.random.default_rng(0)
    noisy = np.where(img > 0, img + rng.integers(-1, 2, img.shape), 0).astype(np.int32)
    frac = [float(api.normal_fraction(normals_ref(img[None], noisy, 5, scenario["K"], step, JUMP, COS30))[0]) for step in (1, 4, 8)]
    print(f"agreement of the scene pose with its own render +-1 mm at steps 1, 4, 8: {frac}")
    assert frac[0] < frac[1]


def test_reference_by_hand():
    """A 7 x 7 slope: defined in the middle only, undefined beside a hole, beside a jump and beside the border; agreement by the angle."""
    K = np.array([100.0, 0, 3.0, 0, 100.0, 3.0, 0, 0, 1], np.float32)
    x = np.arange(7)
    d = np.broadcast_to(1000 + 5 * x, (7, 7)).astype(np.int32).copy()
    defined, a, b, c = normal_of(d, K, 1, 5)
    assert defined[1:6, 1:6].all() and defined.sum() == 25
    assert (a[defined] == -1000.0).all() and (b[defined] == 0).all() and c[3, 3] == 2 * 1015.0      # gu = 10, the principal point
    assert c[3, 4] == 2 * 1020.0 + 10.0
    assert not normal_of(d, K, 1, 4)[0].any()                      # a neighbour 5 mm away needs a jump of 5
    assert normal_of(d, K, 3, 15)[0].sum() == 1 and normal_of(d, K, 4, 100)[0].sum() == 0
    d[3, 3] = 0
    defined = normal_of(d, K, 1, 5)[0]
    assert defined.sum() == 20 and not defined[3, 3] and not defined[2, 3] and not defined[3, 2] and defined[2, 2]
    ext = np.array([[2**31 - 1] * 3, [2**31 - 1, 1, 2**31 - 1], [2**31 - 1] * 3], np.int32)            # differences need 64 bits
    assert not normal_of(ext, K, 1, 2**31 - 3)[0].any() and normal_of(ext, K, 1, 2**31 - 2)[0].sum() == 1
    flat, slope = (np.array([0.0]), np.array([0.0]), np.array([1.0])), (np.array([1.0]), np.array([0.0]), np.array([1.0]))     # 45 degrees apart
    assert agreement(flat, slope, 0.70)[0] and not agreement(flat, slope, 0.71)[0]
    assert agreement(flat, flat, 1.0)[0] and not agreement(flat, (flat[0], flat[1], -flat[2]), 0.0)[0]   # opposite: dot < 0
    d45 = (np.array([1.0]), np.array([0.0]), np.array([0.0]))
    assert agreement(flat, d45, 0.0)[0] and not agreement(flat, d45, 1e-3)[0]                           # a right angle: dot == 0


def _records(rows):
    out = np.zeros(len(rows), api.NORMAL)
    for i, (t, a) in enumerate(rows):
        out[i]["tested"], out[i]["agree"], out[i]["disagree"] = t, a, t - a
    return out


def test_normal_fraction_and_filter():
    rec = _records([(100, 50), (100, 100), (0, 0), (40, 0), (80, 20), (2**32 - 1, 2**31)])
    frac = api.normal_fraction(rec)
    assert frac.dtype == np.float64
    assert frac.tolist() == [0.5, 1.0, 0.0, 0.0, 0.25, 2**31 / (2**32 - 1)]
    order = np.array([4, 1, 0, 5, 3, 2])
    assert api.filter_by_normals(order, rec, 0.5).tolist() == [1, 0, 5]
    assert api.filter_by_normals(order, rec, 0.0).tolist() == order.tolist()
    assert api.filter_by_normals(order, rec, 0.26).dtype == np.int64
    assert api.filter_by_normals(order[:2], rec, 0.3).tolist() == [1]              # a partial order stays partial
    assert api.filter_by_normals(np.zeros(0, np.int64), rec, 0.3).tolist() == []
    assert api.filter_by_normals(order, rec, 1.5).tolist() == []
    scores = np.zeros(3, api.SCORE)
    scores["visible"], scores["inlier"] = [100, 100, 100], [90, 80, 70]
    keep = api.filter_by_normals(api.rank_hypotheses(scores), _records([(80, 10), (70, 60), (60, 55)]), 0.5)
    assert keep.tolist() == [1, 2]                                 # the best-ranked hypothesis faces the wrong way
    assert api.select_hypotheses(scores, np.diag(scores["inlier"]).astype(np.uint32), order=keep).tolist() == [1, 2]


# ---- the argument checks that need no device ---------------------------------------------------------------------------------------------
def test_argument_errors_without_a_device():
    """step, jump_mm and cos_min are checked before any device is touched: PR_ERR_INVALID with or without a GPU, nothing written."""
    lib = _lib.load()
    K = np.ascontiguousarray(synth.K_TEST)
    pj = np.zeros(16, np.float32)
    poses = np.zeros((2, 16), np.float32)
    sc, nr = np.full(2, 7, np.uint8).repeat(32).view(api.SCORE), np.full(2, 7, np.uint8).repeat(32).view(api.NORMAL)
    before = sc.tobytes(), nr.tobytes()
    no_roi = _lib.Roi(0, 0, 0, 0)
    table = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0))
    idx = np.zeros(2, np.uint32)

    def single(step, jump, cos_min, n=2):
        return lib.pr_score_normals(None, 0, poses.ctypes.data, n, 64, 48, pj.ctypes.data, no_roi, None, 1, 5, K.ctypes.data, step, jump, cos_min,
                                    sc.ctypes.data, nr.ctypes.data, None)

    def multi(step, jump, cos_min, n=2):
        return lib.pr_score_normals_multi(table, 1, idx.ctypes.data, poses.ctypes.data, n, 64, 48, pj.ctypes.data, no_roi, None, 1, 5, K.ctypes.data,
                                          step, jump, cos_min, sc.ctypes.data, nr.ctypes.data, None)

    for call, name in ((single, "pr_score_normals"), (multi, "pr_score_normals_multi")):
        for step, jump, cos_min, word in ((0, 20, 0.5, "step"), (api.NORMAL_MAX_STEP + 1, 20, 0.5, "step"), (2**32 - 1, 20, 0.5, "step"), (4, -1, 0.5, "jump_mm"),
                                          (4, -2**31, 0.5, "jump_mm"), (4, 20, -1e-6, "cos_min"), (4, 20, 1.0001, "cos_min"), (4, 20, float("nan"), "cos_min"),
                                          (4, 20, float("inf"), "cos_min")):
            assert call(step, jump, cos_min) == _lib.PR_ERR_INVALID, (name, step, jump, cos_min)
            assert f"{name}: {word}" in lib.pr_last_error().decode()
            assert call(step, jump, cos_min, n=0) == _lib.PR_ERR_INVALID          # ... whatever the number of hypotheses
    assert (sc.tobytes(), nr.tobytes()) == before
    if api.device_count() == 0:                                    # what passes these checks needs a device (there is no CPU fallback)
        for call in (single, multi):
            for step, jump, cos_min in ((1, 0, 0.0), (api.NORMAL_MAX_STEP, 2**31 - 1, 1.0)):
                assert call(step, jump, cos_min) == _lib.PR_ERR_NO_DEVICE
        with pytest.raises(api.PoseRefineError) as e:
            api.score_normals(np.zeros((1, 3, 3), np.float32), np.eye(4, dtype=np.float32)[None], 64, 48, pj, np.zeros((48, 64), np.int32), 5, K, 4, 20, 0.5)
        assert e.value.code == _lib.PR_ERR_NO_DEVICE
    assert (sc.tobytes(), nr.tobytes()) == before
