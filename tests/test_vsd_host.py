"""Host side of the visible surface discrepancy (no GPU): the record's layout, the clauses of the definition by hand on one-row images, the
float32 reference of pr_pose_vsd (tests/vsd_ref.py) against its float64 and integer restatements on the 32-pair small case, the argument
checks -- which come before any device use, so they answer on a box without one --, and vsd_errors / vsd_recall."""
import numpy as np
import pytest

import vsd_ref as R
from pose_refine_amd import _lib, api


def test_record_layout_and_constants():
    d = _lib.VSD
    assert d.itemsize == 64 and _lib.VSD_MAX_TAUS == 12
    assert [d.fields[n][1] for n in ("visib_gt", "visib_est", "inter", "uni", "far")] == [0, 4, 8, 12, 16] and d["far"].shape == (12,)
    assert api.VSD is _lib.VSD and "pr_pose_vsd" in _lib.SIGNATURES and "pr_pose_vsd_multi" in _lib.SIGNATURES
    assert api.VSD_DELTA_BOP == 15.0
    want = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
    assert list(api.VSD_TAUS_BOP) == want and list(api.VSD_THRESHOLDS_BOP) == want


def _rec(vg, ve, inter, uni, far):
    r = np.zeros(1, api.VSD)
    r["visib_gt"], r["visib_est"], r["inter"], r["uni"] = vg, ve, inter, uni
    r["far"][0, :len(far)] = far
    return r


def _one_row(e, g, s, delta, taus, want):
    """A 1 x n image: vsd_ref (K == NULL), vsd_int and the hand-written record agree."""
    e, g, s = (np.array([v], np.int32) for v in (e, g, s))
    a = R.vsd_ref(e[None], g[None], s, None, delta, taus)
    b = R.vsd_int(e[None], g[None], s, delta, taus)
    c = R.vsd_truth64(e[None], g[None], s, None, delta, taus)
    R.assert_vsd_equal(a, want)
    R.assert_vsd_equal(b, want)
    R.assert_vsd_equal(c, want)
    return a


def test_mask_clauses_by_hand():
    # no scene measurement (s <= 0): both visible wherever drawn
    _one_row([500, 500, 0, 0], [500, 0, 500, 0], [0, -3, 0, 0], 15, [10], _rec(2, 2, 1, 3, [0]))
    # the truth occluded by more than delta (scene 16 mm in front): not visible; at exactly delta it is.  The estimate there is judged on its own
    _one_row([0, 0, 516, 515], [516, 515, 516, 516], [500, 500, 500, 500], 15, [1], _rec(1, 1, 0, 2, [0]))
    # the estimate occluded but kept by vg: E - T > delta, yet the truth is visible at that pixel
    _one_row([540, 540], [510, 520], [500, 500], 15, [20, 30, 31], _rec(1, 1, 1, 1, [1, 1, 0]))
    # estimate only / truth only
    _one_row([505, 0], [0, 0], [500, 500], 15, [5], _rec(0, 1, 0, 1, [0]))
    _one_row([0, 0], [0, 505], [500, 500], 15, [5], _rec(1, 0, 0, 1, [0]))
    # |G - E| exactly equal to a tau counts as far (K == NULL: integers); one less does not
    _one_row([500, 500], [508, 507], [500, 500], 15, [8], _rec(2, 2, 2, 2, [1]))
    # tau = 0: far == inter
    _one_row([500, 503, 0], [500, 500, 500], [500, 500, 500], 15, [0, 3, 4], _rec(3, 2, 2, 3, [2, 1, 0]))
    # a surface behind the scene by no more than delta stays visible; the scene far behind both hides nothing
    _one_row([400, 400], [415, 400], [400, 900], 15, [15, 16], _rec(2, 2, 2, 2, [1, 0]))
    # nothing drawn at all: all zero, and the error is 1
    a = _one_row([0, 0, 0], [0, 0, 0], [500, 0, 700], 15, [1, 2], _rec(0, 0, 0, 0, [0, 0]))
    assert np.array_equal(api.vsd_errors(a, 2), [[1.0, 1.0]])


def test_ray_factor_with_k():
    """With K the distances grow with the ray factor: the same depth difference of 8 mm passes tau = 8 off the principal point only."""
    K = np.array([10.0, 0, 0.0, 0, 10.0, 0.0, 0, 0, 1], np.float32)
    e = np.array([[[500, 500]]], np.int32)
    g = np.array([[[508, 508]]], np.int32)
    s = np.zeros((1, 2), np.int32)
    with_k = R.vsd_ref(e, g, s, K, 15, [8.0, 8.03, 8.05])
    # pixel 0: c = 1, |G - E| = 8; pixel 1: c = sqrt(1.01) = 1.004988, |G - E| = 8.0399
    R.assert_vsd_equal(with_k, _rec(2, 2, 2, 2, [2, 1, 0]))
    R.assert_vsd_equal(R.vsd_truth64(e, g, s, K, 15, [8.0, 8.03, 8.05]), with_k)


def test_small_case_float32_equals_float64_and_integers():
    c = R.small_case()
    assert c["W"] == 48 and c["H"] == 32 and len(c["est"]) == 32 and len(c["tris"]) == 12
    a = R.vsd_ref(c["r_est"], c["r_gt"], c["scene"], c["K"], c["delta"], c["taus"])
    R.assert_vsd_equal(a, R.vsd_truth64(c["r_est"], c["r_gt"], c["scene"], c["K"], c["delta"], c["taus"]))      # every count of all 32 pairs
    R.assert_vsd_equal(R.vsd_ref(c["r_est"], c["r_gt"], c["scene"].astype(np.uint16), c["K"], c["delta"], c["taus"]), a)
    n = R.vsd_ref(c["r_est"], c["r_gt"], c["scene"], None, c["delta"], c["taus"])
    R.assert_vsd_equal(n, R.vsd_int(c["r_est"], c["r_gt"], c["scene"], 15, [int(t) for t in c["taus"]]))
    far = a["far"][:, :10].astype(np.int64)
    # the batch exercises what it is meant to: the masks differ, the thresholds cut at different places
    assert (a["visib_gt"] != a["visib_est"]).any() and (a["inter"] < a["uni"]).any() and (far[:, 0] > 0).any()
    assert ((far[:, 0] > far[:, 1]) & (far[:, 1] > far[:, 2]) & (far[:, 2] > 0) & (far[:, -1] == 0)).any()    # far decreasing to 0
    assert (np.diff(far, axis=1) <= 0).all() and (far[:, 0] <= a["inter"]).all() and (far[:, -1] > 0).any()
    assert (a["far"][:, 10:] == 0).all()
    assert (a["uni"].astype(np.int64) == a["visib_gt"].astype(np.int64) + a["visib_est"] - a["inter"]).all()
    assert far.max() >= 100 and ((far > 9) & (far < 100)).any()


def test_errors_and_recall():
    r = np.concatenate([_rec(10, 10, 8, 12, [8, 4, 0]), _rec(0, 0, 0, 0, [0, 0, 0]), _rec(5, 5, 5, 5, [0, 0, 0])])
    e = api.vsd_errors(r, 3)
    assert e.dtype == np.float64 and e.shape == (3, 3)
    assert np.array_equal(e, [[1.0, 8 / 12, 4 / 12], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    assert api.vsd_errors(r, 0).shape == (3, 0)
    assert api.vsd_recall(e, [0.5]) == 4 / 9 and api.vsd_recall(e, [0.0]) == 0.0
    assert api.vsd_recall(e, [0.5, 0.7]) == (4 + 5) / 18
    assert api.vsd_recall(e) == ((e[..., None] < np.array(api.VSD_THRESHOLDS_BOP)).mean())
    with pytest.raises(ValueError):
        api.vsd_errors(r, 13)


# ---- argument checks: before any device is touched ---------------------------------------------------------------------------------
FAKE_DEV = 0x10000                       # a non-null "device pointer" that a correct library never dereferences in these calls
K_OK = np.array([60.0, 0, 23.5, 0, 60.0, 15.5, 0, 0, 1], np.float32)
EYE4 = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))


def _call(multi=False, tris=FAKE_DEV, est="eye", n_est=None, gt="eye", n_gt=None, W=48, H=32, proj="eye", scene=FAKE_DEV, Kc=None, delta=15.0,
          taus="two", n_taus=None, out="buf", meshes="table", n_meshes=1, index="zeros"):
    """pr_pose_vsd (pr_pose_vsd_multi) on four identity pairs unless told otherwise (None: a null pointer); nothing may be written unless it succeeds."""
    est = EYE4 if isinstance(est, str) else est
    gt = EYE4 if isinstance(gt, str) else gt
    proj = np.eye(4, dtype=np.float32) if isinstance(proj, str) else proj
    taus = np.array([5.0, 10.0], np.float32) if isinstance(taus, str) else taus
    buf = np.full(8 * 64, 0xAB, np.uint8)
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)  # noqa: E731
    n = lambda x, given: given if given is not None else (0 if x is None else len(x))  # noqa: E731
    tail = (p(est), n(est, n_est), p(gt), n(gt, n_gt), W, H, p(proj), scene, 1, p(Kc), delta, p(taus), n(taus, n_taus), buf.ctypes.data if out == "buf" else out)
    if multi:
        table = (_lib.MeshRef * 1)(_lib.MeshRef(FAKE_DEV, 12)) if isinstance(meshes, str) else meshes
        idx = np.zeros(max(1, n(est, n_est)), np.uint32) if isinstance(index, str) else index
        rc = _lib.load().pr_pose_vsd_multi(table, n_meshes, p(idx), *tail)
    else:
        rc = _lib.load().pr_pose_vsd(tris, 12, *tail)
    assert (buf == 0xAB).all() or rc == _lib.PR_OK
    return rc


@pytest.mark.parametrize("multi", [False, True])
def test_invalid_arguments_are_rejected_before_any_device_use(multi):
    INV = _lib.PR_ERR_INVALID
    name = "pr_pose_vsd_multi" if multi else "pr_pose_vsd"
    call = lambda **kw: _call(multi=multi, **kw)  # noqa: E731

    def refused(**kw):
        assert call(**kw) == INV, kw
        assert name in _lib.load().pr_last_error().decode() or "frames larger" in _lib.load().pr_last_error().decode()

    refused(gt=EYE4[:3])                                           # n_gt neither n_est nor 1
    refused(gt=EYE4[:0])
    refused(est=EYE4[:1], gt=EYE4[:2])
    if multi:
        refused(gt=EYE4[:1])                                       # a mixed batch takes pairs only
    refused(taus=np.arange(13, dtype=np.float32))                  # n_taus > 12
    refused(taus=None, n_taus=2)                                   # taus announced, none given
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        refused(delta=bad)
        refused(taus=np.array([1.0, bad], np.float32))
        if not np.isfinite(bad):
            kc = K_OK.copy()
            kc[7] = bad                                            # an entry the ray factor never reads: every entry is checked
            refused(Kc=kc)
            for where in ("est", "gt"):
                m = EYE4.copy()
                m[2, 1, 3] = bad
                refused(**{where: m})
    refused(taus=np.array([1.0, 3.0, 2.0], np.float32))            # taus must not decrease
    assert call(taus=np.array([2.0, 2.0, 2.0], np.float32), n_est=0, n_gt=0) == _lib.PR_OK
    for i in (0, 4):
        kc = K_OK.copy()
        kc[i] = 0.0
        refused(Kc=kc)
    refused(proj=None)
    refused(est=None, n_est=4)
    refused(gt=None, n_gt=4)
    refused(scene=None)
    refused(out=None)
    if not multi:
        refused(tris=None)
    for w, h in ((0, 32), (48, 0), (8193, 1), (8192, 4096)):       # the frame-size check of the scoring calls
        refused(W=w, H=h)
    if multi:                                                      # the mesh table's own checks need no device either
        refused(meshes=None)
        refused(n_meshes=0)
        refused(index=None)
        refused(index=np.array([0, 0, 1, 0], np.uint32))
        refused(meshes=(_lib.MeshRef * 1)(_lib.MeshRef(None, 12)))
    # nothing to compute: PR_OK without a device, without arrays
    assert call(est=None, gt=None, proj=None, scene=None, taus=None, n_taus=0, out=None, tris=None, meshes=None, n_meshes=0, index=None) == _lib.PR_OK
    if not multi:
        assert call(est=None, gt=EYE4[:1], Kc=K_OK) == _lib.PR_OK   # no estimates against one truth
    if api.device_count() == 0:                                    # ... and a valid call does ask for the device
        assert call() == _lib.PR_ERR_NO_DEVICE and call(Kc=K_OK, taus=None, n_taus=0) == _lib.PR_ERR_NO_DEVICE
        if not multi:
            assert call(gt=EYE4[:1]) == _lib.PR_ERR_NO_DEVICE


def test_api_checks_shapes():
    tris, scene = np.zeros((1, 3, 3), np.float32), np.zeros((32, 48), np.int32)
    with pytest.raises(ValueError):
        api.pose_vsd(tris, EYE4, np.zeros((2, 3, 4), np.float32), 48, 32, np.eye(4), scene)
    with pytest.raises(ValueError):
        api.pose_vsd(tris, EYE4, EYE4, 48, 32, np.eye(4), scene, K=np.ones(8, np.float32))
