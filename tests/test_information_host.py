"""Host tests (no GPU) of pose observability (pr_pose_info / pr_pose_eig, include/pose_refine.h): the float64 reference (tests/info_ref.py) on
analytic surfaces, pr_info_covariance against numpy.linalg.pinv, the argument errors of the four entry points, and the records' layouts.

The bound on a null eigenvalue (info_ref.null_bound).  Let v be a unit vector of the analytic null space: with exact points s, unit normals n and
centre c every row J = ((s - c) x n / rho, n) satisfies J v = 0.  The inputs reach the pass as float32: s, n and c each move by at most 2^-24 of
their magnitude, so with q = s - c
    |delta (q x n)| <= |delta q| |n| + |q| |delta n| <= (2^-24 |s| + 2^-24 |c|) + |q| 2^-24 <= 3 * 2^-24 max|s|        (|c|, |q| <= max|s|)
    |delta n|       <= 2^-24                                                                <= 2^-24 max|s| / rho       (rho <= max|s| here)
and |delta J v| <= |delta a| + |delta n| <= 4 * 2^-24 max|s| / rho.  Then v^T H v = sum w (delta J v)^2 <= (4 * 2^-24 max|s| / rho)^2 sum w for every
unit v of that subspace, and by Courant-Fischer the dim-th smallest eigenvalue of H is no larger.  (The float64 arithmetic after the rounding adds
2^-53-sized terms, nine decades below.)"""
import ctypes as C
import os

import numpy as np
import pytest

import info_ref as I
import robust_ref as R
from pose_refine_amd import _lib, api

F32, F64 = np.float32, np.float64


# ---- (a) the reference on analytic surfaces ---------------------------------------------------------------------------------------------------
def reference_eig(points, normals, c, rho, robust=None, offset=0.001):
    """The cloud = the surface's float32 points moved `offset` along their normals; the scene = the points themselves with their normals."""
    d, n = points.astype(F32), normals.astype(F32)
    cloud = (points + offset * normals).astype(F32)
    corr = (d, n, np.ones(len(d), bool))
    rec = I.record(cloud, corr, robust, c, rho)
    lam, V = I.eigh(rec["sums"][:21])
    return rec, lam, V, float(np.abs(cloud).max())


CASES = {"plane": (I.plane_cloud, (0.0, 0.0, 0.8), 0.1, 3), "sphere": (I.sphere_cloud, (0.02, -0.01, 0.8), 0.05, 3),
         "cylinder": (I.cylinder_cloud, (0.0, 0.0, 0.8), 0.04, 2)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_null_spaces_of_analytic_surfaces(name):
    make, c, rho, dim = CASES[name]
    p, nr, proj = make(5000)
    if name == "plane":
        p = p - 0.001 * nr                                           # the moved cloud lies ON the plane z = 0.8, where the centre is
    rec, lam, V, smax = reference_eig(p, nr, c, rho)
    assert rec["n_valid"] == 5000 and rec["n_zero_weight"] == 0
    bound = I.null_bound(smax, rho, rec["sums"][27])
    assert (np.abs(lam[:dim]) <= bound).all(), (name, lam[:dim], bound)
    assert lam[dim] > 1e-4 * lam[5] and lam[dim] > 1e6 * bound, (name, lam)      # the constrained directions stand ten decades clear of the null ones
    assert np.abs(I.projector(V, range(dim)) - proj).max() <= 1e-6, name
    print(name, "lambda / lambda[5]", lam / lam[5], "bound / lambda[5]", bound / lam[5])


def test_reference_generic_cloud_has_full_rank():
    g = np.random.default_rng(7)
    p = np.array([0.0, 0.0, 0.8]) + g.uniform(-0.05, 0.05, (4000, 3))
    nr = g.normal(size=(4000, 3))
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    rec, lam, V, _ = reference_eig(p, nr, (0.0, 0.0, 0.8), 0.05)
    assert I.rank_of(lam, 1e-3) == 6 and lam[0] > 0.05 * lam[5]


def test_reference_weights_and_zero_weight_count():
    p, nr, _ = I.sphere_cloud(400)
    d, n = p.astype(F32), nr.astype(F32)
    off = np.where(np.arange(400) % 4 == 0, 0.02, 0.001)[:, None]   # every fourth point 20 mm off: beyond a 5 mm Tukey scale
    cloud = (p + off * nr).astype(F32)
    corr = (d, n, np.arange(400) % 10 != 9)                          # every tenth without a correspondence
    rb = R.describe(R.TUKEY, 0.005)
    rec = I.record(cloud, corr, rb, (0.02, -0.01, 0.8), 0.05)
    t, w, r = I.terms(cloud, corr, rb, (0.02, -0.01, 0.8), 0.05)
    assert rec["n_points"] == 400 and rec["n_valid"] == 360 and rec["n_zero_weight"] == int((np.abs(r) >= F32(0.005)).sum()) > 0
    assert np.array_equal(t[:, 27], w.astype(F64)) and np.array_equal(t[:, 28], (w.astype(F64) * r.astype(F64)) * r.astype(F64))
    plain = I.record(cloud, corr, None, (0.02, -0.01, 0.8), 0.05)
    assert plain["sums"][27] == 360.0 and plain["n_zero_weight"] == 0 and plain["sums"][28] == plain["sums"][29]


# ---- (b) pr_info_covariance -------------------------------------------------------------------------------------------------------------------
def records_of(name, n=2000):
    make, c, rho, dim = CASES[name]
    p, nr, _ = make(n)
    rec, lam, V, _ = reference_eig(p, nr, c, rho)
    info, eig = np.zeros(1, _lib.POSE_INFO), np.zeros(1, _lib.POSE_EIG)
    info["n_points"] = info["n_valid"] = n
    info["c"], info["rho"] = c, rho
    info["H"], info["g"] = rec["sums"][:21], rec["sums"][21:27]
    info["sum_w"], info["sum_wr2"], info["sum_r2"] = rec["sums"][27:30]
    eig["lambda"], eig["V"] = lam, V
    return info[0], eig[0], dim


@pytest.mark.parametrize("name", sorted(CASES))
def test_covariance_is_the_pseudo_inverse_on_the_observable_directions(name):
    info, eig, dim = records_of(name)
    H = I.sym6(info["H"])
    for sigma in (None, 0.001):
        cov, rank, s2 = api.pose_covariance(info, eig, 1e-9, sigma=sigma, physical=False)
        want_s2 = 1e-6 if sigma else I.residual_sigma2(float(info["sum_wr2"]), float(info["sum_w"]), int(info["n_valid"]))
        assert rank == 6 - dim and s2 == pytest.approx(want_s2, rel=1e-15)
        pinv = np.linalg.pinv(H, rcond=1e-9, hermitian=True)
        assert np.abs(cov - s2 * pinv).max() <= 1e-9 * np.abs(s2 * pinv).max(), (name, sigma)
        ref, rrank = I.covariance(eig["lambda"], eig["V"], s2, 1e-9)
        assert rrank == rank and np.abs(cov - ref).max() <= 1e-14 * np.abs(ref).max()
        phys, _, _ = api.pose_covariance(info, eig, 1e-9, sigma=sigma)
        sc = np.array([1 / float(info["rho"])] * 3 + [1.0] * 3)
        assert np.allclose(phys, cov * sc[:, None] * sc[None, :], rtol=1e-15, atol=0)


def test_covariance_rank_cut_and_helpers():
    info, eig, _ = records_of("plane")
    eig = eig.copy()
    eig["lambda"] = [0.0, -1e-20, 1e-9, 1e-3, 0.5, 1.0]
    eig["V"] = np.eye(6)
    for ratio, want in ((0.0, 4), (1e-9, 3), (1e-6, 3), (1e-3, 2), (0.5, 1), (1.0, 0)):      # strict '>' against min_ratio * lambda[5]
        cov, rank, _ = api.pose_covariance(info, eig, ratio, sigma=1.0, physical=False)
        assert rank == want == I.rank_of(eig["lambda"], ratio) == int(api.observable_rank(eig, ratio)[0]), ratio
        lam = np.asarray(eig["lambda"])
        keep = (lam > 0) & (lam > ratio * lam[5])
        assert np.array_equal(np.diag(cov), np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)) and not (cov - np.diag(np.diag(cov))).any()
    both = np.array([eig, eig], _lib.POSE_EIG)
    both["lambda"][1] = [1, 1, 1, 1, 1, 1]
    assert list(api.observable_rank(both, 1e-6)) == [3, 6]
    assert list(api.filter_by_observability([1, 0], both, 1e-6)) == [1] and list(api.filter_by_observability([1, 0], both, 1e-6, min_rank=3)) == [1, 0]
    w, t = api.weakest_twist(info, eig, k=2)
    assert np.array_equal(w, [0, 0, 1 / float(info["rho"])]) and not t.any()


def test_covariance_errors():
    info, eig, _ = records_of("sphere")
    lib = _lib.load()
    cov = np.full(21, 7.0)
    rank, s2 = C.c_uint32(9), C.c_double(9.0)

    def call(i, e, sigma, ratio):
        return lib.pr_info_covariance(i, e, sigma, ratio, _lib.ptr(cov), C.byref(rank), C.byref(s2))
    i1, e1 = np.array([info], _lib.POSE_INFO), np.array([eig], _lib.POSE_EIG)
    assert call(None, _lib.ptr(e1), 1.0, 0.0) == _lib.PR_ERR_INVALID and call(_lib.ptr(i1), None, 1.0, 0.0) == _lib.PR_ERR_INVALID
    for ratio in (-1e-9, float("nan"), float("inf")):
        assert call(_lib.ptr(i1), _lib.ptr(e1), 1.0, ratio) == _lib.PR_ERR_INVALID
    assert call(_lib.ptr(i1), _lib.ptr(e1), float("nan"), 0.0) == _lib.PR_ERR_INVALID
    few, empty = i1.copy(), i1.copy()
    few["n_valid"] = 6
    empty["sum_w"] = 0.0
    for sigma in (0.0, -1.0):
        assert call(_lib.ptr(few), _lib.ptr(e1), sigma, 0.0) == _lib.PR_ERR_INVALID and call(_lib.ptr(empty), _lib.ptr(e1), sigma, 0.0) == _lib.PR_ERR_INVALID
    assert (cov == 7.0).all() and rank.value == 9 and s2.value == 9.0
    assert call(_lib.ptr(few), _lib.ptr(e1), 0.002, 0.0) == _lib.PR_OK and s2.value == 0.002 * 0.002      # a given sigma needs no residuals
    few["n_valid"] = 7
    assert call(_lib.ptr(few), _lib.ptr(e1), 0.0, 0.0) == _lib.PR_OK and s2.value == pytest.approx(float(info["sum_wr2"]) / float(info["sum_w"]) * 7.0)
    assert lib.pr_info_covariance(_lib.ptr(i1), _lib.ptr(e1), 1.0, 0.0, None, None, None) == _lib.PR_OK


# ---- (c) argument errors, before any device is looked for -------------------------------------------------------------------------------------
class Args:
    """Host buffers that stand in for every pointer of a call (never dereferenced on the device: each call below is refused first)."""

    def __init__(self):
        self.poses = np.tile(np.eye(4, dtype=F32).reshape(16), (2, 1))
        self.proj = np.eye(4, dtype=F32).reshape(16)
        self.K = np.array([500, 0, 32, 0, 500, 24, 0, 0, 1], F32)
        self.scene = _lib.SceneProjDesc()
        self.offs = np.array([0, 4, 8], np.uint32)
        self.centers = np.array([[0, 0, 0.8], [0, 0, 0.8]], F32)
        self.radii = np.array([0.05, 0.05], F32)
        self.center_model = np.zeros(3, F32)
        self.meshes = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0))
        self.idx = np.zeros(2, np.uint32)
        self.info = np.full(2 * 272, 7, np.uint8).view(_lib.POSE_INFO)
        self.eig = np.full(2 * 344, 7, np.uint8).view(_lib.POSE_EIG)
        self.sizes = np.full(2, 7, np.uint32)
        self.cloud_dev = 0x1000                                      # (a value that is not NULL; no refused call reads it)
        self.robust = None
        self.kind = _lib.SCENE_PROJ
        self.radius = 0.05
        self.wh = (64, 48)
        self.roi = (0, 0, 0, 0)

    def _p(self, null):
        return lambda name, v: None if name in null else v

    def icp(self, debug=False, **null):
        p = self._p(null)
        head = (p("cloud", self.cloud_dev), p("offs", _lib.ptr(self.offs)), 2, self.kind, p("scene", C.addressof(self.scene)))
        tail = (self.robust, p("centers", _lib.ptr(self.centers)), p("radii", _lib.ptr(self.radii)), p("info", _lib.ptr(self.info)), _lib.ptr(self.eig))
        return _lib.load().pr_debug_icp_information(*head, 1, *tail) if debug else _lib.load().pr_icp_information(*head, *tail)

    def pose(self, **null):
        p = self._p(null)
        return _lib.load().pr_pose_information(None, 0, p("poses", _lib.ptr(self.poses)), 2, *self.wh, p("proj", _lib.ptr(self.proj)), p("K", _lib.ptr(self.K)),
                                               self.kind, p("scene", C.addressof(self.scene)), _lib.Roi(*self.roi), self.robust,
                                               p("centers", _lib.ptr(self.center_model)), self.radius, p("info", _lib.ptr(self.info)), _lib.ptr(self.eig),
                                               _lib.ptr(self.sizes))

    def multi(self, **null):
        p = self._p(null)
        return _lib.load().pr_pose_information_multi(p("meshes", self.meshes), 1, p("idx", _lib.ptr(self.idx)), p("poses", _lib.ptr(self.poses)), 2, *self.wh,
                                                     p("proj", _lib.ptr(self.proj)), p("K", _lib.ptr(self.K)), self.kind, p("scene", C.addressof(self.scene)),
                                                     _lib.Roi(*self.roi), self.robust, p("centers", _lib.ptr(self.center_model)),
                                                     p("radii", _lib.ptr(self.radii)), p("info", _lib.ptr(self.info)), _lib.ptr(self.eig), _lib.ptr(self.sizes))

    def all_refuse(self, what, fused_only=False, cloud_only=False):
        calls = ([] if fused_only else [self.icp, lambda **k: self.icp(debug=True, **k)]) + ([] if cloud_only else [self.pose, self.multi])
        for call in calls:
            assert call() == _lib.PR_ERR_INVALID, what
        self.untouched()

    def untouched(self):
        assert (self.info.view(np.uint8) == 7).all() and (self.eig.view(np.uint8) == 7).all() and (self.sizes == 7).all()


def test_entry_points_refuse_null_pointers():
    a = Args()
    for name in ("offs", "scene", "centers", "radii", "info"):
        assert a.icp(**{name: True}) == _lib.PR_ERR_INVALID and a.icp(debug=True, **{name: True}) == _lib.PR_ERR_INVALID, name
    assert a.icp(cloud=True) == _lib.PR_ERR_INVALID                  # no array, but points
    for name in ("poses", "proj", "K", "scene", "centers", "info"):
        assert a.pose(**{name: True}) == _lib.PR_ERR_INVALID and a.multi(**{name: True}) == _lib.PR_ERR_INVALID, name
    for name in ("meshes", "idx", "radii"):
        assert a.multi(**{name: True}) == _lib.PR_ERR_INVALID, name
    a.untouched()


@pytest.mark.parametrize("what", ["unknown kind", "reserved", "c zero", "c nan", "inv_c recomputed"])
def test_entry_points_refuse_a_bad_descriptor(what):
    g = api.Robust(R.HUBER, 0.005).desc()
    bad = {"unknown kind": _lib.RobustDesc(7, g.c, g.inv_c, 0), "reserved": _lib.RobustDesc(g.kind, g.c, g.inv_c, 1),
           "c zero": _lib.RobustDesc(g.kind, 0.0, 0.0, 0), "c nan": _lib.RobustDesc(g.kind, float("nan"), g.inv_c, 0),
           "inv_c recomputed": _lib.RobustDesc(g.kind, g.c, float(np.nextafter(F32(g.inv_c), F32(0))), 0)}[what]
    a = Args()
    a.robust = C.addressof(bad)
    a.all_refuse(what)
    assert b"pr_robust" in _lib.load().pr_last_error()


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_entry_points_refuse_a_centre_that_is_not_finite(value):
    a = Args()
    a.centers[1, 2] = value
    a.center_model[1] = value
    a.all_refuse(value)
    b = Args()
    b.poses[1, 7] = value                                            # a pose that sends the model's centre nowhere
    b.all_refuse(value, fused_only=True)


@pytest.mark.parametrize("value", [0.0, -0.05, float("nan"), float("inf")])
def test_entry_points_refuse_a_bad_radius(value):
    a = Args()
    a.radii[0] = value
    a.radius = value
    a.all_refuse(value)


def test_entry_points_refuse_what_the_calls_they_follow_refuse():
    a = Args()
    a.offs[:] = [0, 8, 4]                                            # pr_icp_batch: offsets must not decrease
    a.all_refuse("offsets", cloud_only=True)
    a = Args()
    a.kind = 9
    a.all_refuse("scene kind")
    a = Args()
    a.kind, a.scene = _lib.SCENE_GRID, _lib.SceneGridDesc()          # a grid nobody described
    a.all_refuse("grid descriptor")
    a = Args()
    a.wh = (0, 48)                                                   # pr_refine_batch_roi: an empty frame, a window outside it
    a.all_refuse("frame", fused_only=True)
    a = Args()
    a.roi = (60, 0, 10, 10)
    a.all_refuse("roi", fused_only=True)
    a = Args()
    a.idx[1] = 1                                                     # one mesh in the table
    assert a.multi() == _lib.PR_ERR_INVALID
    a.untouched()


def test_python_wrappers_refuse_what_they_can_see():
    with pytest.raises(ValueError):
        api.pose_information(np.zeros((1, 3, 3), F32), np.eye(4, dtype=F32)[None], 64, 48, np.eye(4, dtype=F32), np.eye(3, dtype=F32), None)      # no Model: no default centre
    with pytest.raises(ValueError):
        api._robust_ptr("huber")


# ---- (d) layouts ----------------------------------------------------------------------------------------------------------------------------
def test_record_layouts_are_the_header_s():
    i, e = _lib.POSE_INFO, _lib.POSE_EIG
    assert i.itemsize == 272 and e.itemsize == 344
    assert {k: i.fields[k][1] for k in i.names} == dict(n_points=0, n_valid=4, n_zero_weight=8, reserved=12, c=16, rho=28, H=32, g=200, sum_w=248,
                                                        sum_wr2=256, sum_r2=264)
    assert {k: e.fields[k][1] for k in e.names} == {"lambda": 0, "V": 48, "sweeps": 336, "reserved": 340}
    assert i["H"].shape == (21,) and e["V"].shape == (6, 6) and _lib.INFO_MAX_SWEEPS == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pose_refine.h")).read()
    assert "#define PR_INFO_MAX_SWEEPS 16" in header and "pr_pose_info (272 B)" in header and "pr_pose_eig (344 B)" in header
