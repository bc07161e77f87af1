"""Host tests of the robust ICP weights (pr_robust, include/pose_refine.h): the descriptor, the argument checks of every _robust entry point
(refused before a device is looked for), the numpy float32 reference of the weight against the float64 formulas, the identity w == 1, and one
behavioural case on the float64 restatement of the loop.  None of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import grid_ref
import robust_ref as R
import truth_ref as T
from pass_sums_ref import u32
from pose_refine_amd import _lib, api

F32 = np.float32
KINDS = (R.HUBER, R.TUKEY, R.CAUCHY)
KIND_NAMES = {R.HUBER: "huber", R.TUKEY: "tukey", R.CAUCHY: "cauchy"}


# ---- 1. pr_robust_describe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.002, 0.005, 0.01, 0.02, 1.0e6, 3.0, 1.0 / 3.0, 1.17549435e-38 * 8, 1.0e30])
def test_describe_computes_inv_c_once_in_float32(c):
    for kind in KINDS:
        rb = api.Robust(kind, c)
        assert rb.kind == kind and u32(rb.c) == u32(F32(c)) and rb.desc().reserved == 0
        assert u32(rb.inv_c) == u32(F32(1) / F32(c))
        ref = R.describe(kind, c)
        assert u32(ref.c) == u32(rb.c) and u32(ref.inv_c) == u32(rb.inv_c)
    none = api.Robust(api.ROBUST_NONE, c)
    assert none.kind == 0 and none.desc().reserved == 0


@pytest.mark.parametrize("kind, c", [(4, 0.01), (0xFFFFFFFF, 0.01), (17, float("nan"))] +
                         [(k, c) for k in KINDS for c in (0.0, -0.0, -0.005, float("nan"), float("inf"), -float("inf"))])
def test_describe_refuses(kind, c):
    out = _lib.RobustDesc(9, 9.0, 9.0, 9)
    rc = _lib.load().pr_robust_describe(kind, c, C.addressof(out))
    assert rc == _lib.PR_ERR_INVALID
    assert (out.kind, out.c, out.inv_c, out.reserved) == (9, 9.0, 9.0, 9)      # nothing written
    with pytest.raises(api.PoseRefineError) as e:
        api.Robust(kind, c)
    assert e.value.code == _lib.PR_ERR_INVALID


def test_describe_refuses_a_null_out_and_none_ignores_c():
    assert _lib.load().pr_robust_describe(R.HUBER, 0.01, None) == _lib.PR_ERR_INVALID
    assert api.Robust(api.ROBUST_NONE, float("nan")).kind == 0            # a kind without a scale does not look at c


# ---- 2. the _robust entry points refuse bad arguments before they look for a device ---------------------------------------------------------
GOOD = api.Robust(R.HUBER, 0.005)


def bad_descriptors():
    g = GOOD.desc()
    return {"unknown kind": _lib.RobustDesc(7, g.c, g.inv_c, 0), "reserved": _lib.RobustDesc(g.kind, g.c, g.inv_c, 1),
            "c zero": _lib.RobustDesc(g.kind, 0.0, 0.0, 0), "c negative": _lib.RobustDesc(g.kind, -g.c, -g.inv_c, 0),
            "c nan": _lib.RobustDesc(g.kind, float("nan"), g.inv_c, 0), "c inf": _lib.RobustDesc(g.kind, float("inf"), 0.0, 0),
            "inv_c recomputed": _lib.RobustDesc(g.kind, g.c, float(np.nextafter(F32(g.inv_c), F32(0))), 0)}


class Args:
    """Host buffers that stand in for every pointer of a call (never dereferenced: each call below is refused first)."""

    def __init__(self, n_levels=1):
        self.poses = np.tile(np.eye(4, dtype=F32).reshape(16), (2, 1))
        self.proj = np.eye(4, dtype=F32).reshape(16)
        self.K = np.array([500, 0, 32, 0, 500, 24, 0, 0, 1], F32)
        self.scene = _lib.SceneProjDesc()
        self.levels = (_lib.PyramidLevel * n_levels)(*[_lib.PyramidLevel(1, _lib.Criteria(0, 0, 1)) for _ in range(n_levels)])
        self.n_levels = n_levels
        self.res = np.full(2, 7, np.uint8).repeat(72).view(_lib.RESULT)
        self.before = self.res.tobytes()
        self.meshes = (_lib.MeshRef * 1)(_lib.MeshRef(None, 0))
        self.idx = np.zeros(2, np.uint32)
        self.offs = np.array([0, 4], np.uint32)
        self.terms = np.full((4, 29), 7, F32)
        self.cloud_dev = 0x1000                                      # (a value that is not NULL; no refused call reads it)

    def pyramid(self, robust, n_robust, **null):
        p = lambda name, v: None if name in null else v
        return _lib.load().pr_refine_pyramid_robust(None, 0, p("poses", _lib.ptr(self.poses)), 2, 64, 48, p("proj", _lib.ptr(self.proj)), p("K", _lib.ptr(self.K)),
                                                    _lib.SCENE_PROJ, p("scene", C.addressof(self.scene)), p("levels", self.levels), self.n_levels,
                                                    _lib.Roi(0, 0, 0, 0), p("res", _lib.ptr(self.res)), None, None, robust, n_robust)

    def pyramid_multi(self, robust, n_robust, **null):
        p = lambda name, v: None if name in null else v
        return _lib.load().pr_refine_pyramid_robust_multi(p("meshes", self.meshes), 1, p("idx", _lib.ptr(self.idx)), p("poses", _lib.ptr(self.poses)), 2, 64, 48,
                                                          p("proj", _lib.ptr(self.proj)), p("K", _lib.ptr(self.K)), _lib.SCENE_PROJ, p("scene", C.addressof(self.scene)),
                                                          p("levels", self.levels), self.n_levels, _lib.Roi(0, 0, 0, 0), p("res", _lib.ptr(self.res)), None, None,
                                                          robust, n_robust)

    def icp(self, robust, **null):
        p = lambda name, v: None if name in null else v
        return _lib.load().pr_icp_batch_robust(self.cloud_dev, p("offs", _lib.ptr(self.offs)), 1, _lib.SCENE_PROJ, p("scene", C.addressof(self.scene)),
                                               _lib.Criteria(0, 0, 1), robust, p("res", _lib.ptr(self.res)))

    def terms_call(self, robust, **null):
        p = lambda name, v: None if name in null else v
        return _lib.load().pr_debug_robust_terms(p("cloud", self.cloud_dev), 4, _lib.SCENE_PROJ, p("scene", C.addressof(self.scene)), None, 0, robust,
                                                 p("terms", _lib.ptr(self.terms)), None)

    def untouched(self):
        return self.res.tobytes() == self.before and (self.terms == 7).all()


@pytest.mark.parametrize("what", sorted(bad_descriptors()))
def test_entry_points_refuse_a_bad_descriptor(what):
    bad = bad_descriptors()[what]
    a = Args()
    for call in (lambda: a.pyramid(C.addressof(bad), 1), lambda: a.pyramid_multi(C.addressof(bad), 1), lambda: a.icp(C.addressof(bad)),
                 lambda: a.terms_call(C.addressof(bad))):
        assert call() == _lib.PR_ERR_INVALID, what
        assert b"pr_robust" in _lib.load().pr_last_error()
    assert a.untouched()
    # ... also as the second entry of a per-level table
    a2 = Args(n_levels=2)
    table = (_lib.RobustDesc * 2)(GOOD.desc(), bad)
    assert a2.pyramid(table, 2) == _lib.PR_ERR_INVALID and a2.pyramid_multi(table, 2) == _lib.PR_ERR_INVALID and a2.untouched()


@pytest.mark.parametrize("n_levels, n_robust", [(1, 0), (1, 2), (3, 2), (3, 4), (2, 0), (4, 3)])
def test_pyramid_calls_refuse_a_table_of_another_length(n_levels, n_robust):
    a = Args(n_levels)
    table = (_lib.RobustDesc * 4)(*[GOOD.desc()] * 4)
    assert a.pyramid(table, n_robust) == _lib.PR_ERR_INVALID and b"n_robust" in _lib.load().pr_last_error()
    assert a.pyramid_multi(table, n_robust) == _lib.PR_ERR_INVALID and b"n_robust" in _lib.load().pr_last_error()
    assert a.untouched()


def test_entry_points_refuse_null_pointers():
    a = Args()
    g = C.addressof(GOOD.desc())
    assert a.pyramid(None, 1) == _lib.PR_ERR_INVALID and a.pyramid_multi(None, 1) == _lib.PR_ERR_INVALID
    assert a.icp(None) == _lib.PR_ERR_INVALID and a.terms_call(None) == _lib.PR_ERR_INVALID
    for name in ("poses", "proj", "K", "scene", "levels", "res"):
        assert a.pyramid(g, 1, **{name: True}) == _lib.PR_ERR_INVALID, name
        assert a.pyramid_multi(g, 1, **{name: True}) == _lib.PR_ERR_INVALID, name
    for name in ("meshes", "idx"):
        assert a.pyramid_multi(g, 1, **{name: True}) == _lib.PR_ERR_INVALID, name
    for name in ("offs", "scene", "res"):
        assert a.icp(g, **{name: True}) == _lib.PR_ERR_INVALID, name
    for name in ("cloud", "scene", "terms"):
        assert a.terms_call(g, **{name: True}) == _lib.PR_ERR_INVALID, name
    assert a.untouched()
    with pytest.raises(ValueError):
        api._robust_table([GOOD, GOOD], 3)
    with pytest.raises(ValueError):
        api._robust_table([], 1)


# ---- 3. the reference's weight against the float64 formulas -----------------------------------------------------------------------------
def sweep(c):
    """Residuals around everything the weight's definition distinguishes: 0, +-c exactly, the float32 neighbours of +-c, a dense band about c,
    eight decades either side, |r| >> c, both signs."""
    c = F32(c)
    near = [c, np.nextafter(c, F32(0)), np.nextafter(c, F32(np.inf)), np.nextafter(np.nextafter(c, F32(0)), F32(0)), np.nextafter(np.nextafter(c, F32(np.inf)), F32(np.inf))]
    band = (c * np.linspace(0.5, 2.0, 301)).astype(F32)
    decades = (c * np.logspace(-8, 8, 321)).astype(F32)
    far = np.array([c * F32(1.0e12), F32(1.0e30)], F32)
    pos = np.concatenate([np.array(near, F32), band, decades, far])
    return np.concatenate([np.zeros(1, F32), pos, -pos]).astype(F32)


def weight64(r, kind, c):
    """The formulas in float64, on the float32 residuals and the float32 scale."""
    r, c = np.asarray(r, np.float64), float(F32(c))
    a = np.abs(r)
    if kind == R.HUBER:
        with np.errstate(divide="ignore"):
            return np.where(a <= c, 1.0, c / a)
    q = (r / c) ** 2
    return np.where(q < 1.0, (1.0 - q) ** 2, 0.0) if kind == R.TUKEY else 1.0 / (1.0 + q)


# measured on the sweep below (largest over c = 2, 5, 10, 20 mm and 1 m), and the bounds the test allows: twice that
HUBER_REL_MEASURED, HUBER_REL_BOUND = 5.60e-8, 1.12e-7
CAUCHY_REL_MEASURED, CAUCHY_REL_BOUND = 1.86e-7, 3.72e-7
TUKEY_ABS_MEASURED, TUKEY_ABS_BOUND = 1.18e-7, 2.36e-7
TUKEY_REL_MEASURED, TUKEY_REL_BOUND = 4.51e-6, 9.02e-6
TINY = float(np.finfo(F32).tiny)          # below float32's normal range a weight has no relative precision left: there the absolute error is held to TINY


@pytest.mark.parametrize("c", [0.002, 0.005, 0.01, 0.02, 1.0])
def test_reference_weight_follows_the_float64_formulas(c):
    """robust_ref.weight (float32, inv_c rounded once) against the float64 formulas over sweep(c).  The bounds are the reference's own error,
    measured on this sweep, times two:
      Huber   largest relative error 5.60e-8 (one rounding of the division), allowed 1.12e-7
      Cauchy  largest relative error 1.86e-7 (inv_c, u, q, 1 + q and the division each round once), allowed 3.72e-7; where the float64 weight
              is below float32's normal range (|r| = 1e30: q overflows, w = 0) the absolute error, at most 1e-60, is held to FLT_MIN
      Tukey   largest absolute error 1.18e-7, allowed 2.36e-7 -- w lies in [0, 1] and (1 - q) cancels as |r| approaches c, so close to c a relative
              figure measures the rounding of q (a few 2^-24) against a weight that goes to zero (0.64 at the float32 neighbour of c); where
              q <= 0.99 the largest relative error is 4.51e-6 (that rounding of q, amplified by 2 q / (1 - q) <= 200), allowed 9.02e-6
    Exact cases: w == 1 inside Huber's band (|r| <= c, the end points included), w == 0 at and beyond Tukey's c, w(0) == 1 for every kind,
    w(-r) == w(r)."""
    r = sweep(c)
    c32 = F32(c)
    for kind in KINDS:
        rb = R.describe(kind, c)
        w = R.weight(r, rb)
        assert w.dtype == F32 and w.shape == r.shape
        w64 = weight64(r, kind, c)
        err = np.abs(w.astype(np.float64) - w64)
        normal = w64 >= TINY
        rel = np.where(normal, err / np.where(normal, w64, 1.0), 0.0)
        assert (err[~normal] <= TINY).all()
        print(f"{KIND_NAMES[kind]} c = {c}: largest relative error {rel.max():.3g}, largest absolute error {err.max():.3g}")
        half = (len(r) - 1) // 2
        assert np.array_equal(u32(w[1:1 + half]), u32(w[1 + half:])), "w(-r) != w(r)"
        assert w[0] == 1.0
        if kind == R.HUBER:
            assert rel.max() <= HUBER_REL_BOUND
            assert (w[np.abs(r) <= c32] == 1.0).all() and (w[np.abs(r) > c32] < 1.0).all()
        elif kind == R.CAUCHY:
            assert rel.max() <= CAUCHY_REL_BOUND
        else:
            assert err.max() <= TUKEY_ABS_BOUND
            q64 = (r.astype(np.float64) / float(c32)) ** 2
            assert rel[q64 <= 0.99].max() <= TUKEY_REL_BOUND
            assert (w[np.abs(r) >= c32] == 0.0).all()
            assert (w[np.abs(r) < np.nextafter(c32, F32(0))] > 0.0).all()


# ---- 4. w == 1 is the plain pass ------------------------------------------------------------------------------------------------------------
def synthetic_corr(n=3000, seed=11):
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-0.3, 0.3, (n, 3)).astype(F32) + F32([0, 0, 0.6])
    d = (cloud + rng.normal(0, 0.01, (n, 3))).astype(F32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    valid = rng.uniform(size=n) < 0.8
    return cloud, (d, nrm, valid)


@pytest.mark.parametrize("kind", KINDS + (R.NONE,))
def test_unit_weight_gives_the_plain_terms(kind):
    cloud, corr = synthetic_corr()
    rb = R.describe(kind, 1.0e6)
    terms, w = R.weighted_terms29(cloud, corr, rb)
    assert (w[corr[2]] == 1.0).all() and (w[~corr[2]] == 0.0).all()
    plain = R.plain_terms29(cloud, corr)
    assert np.array_equal(u32(terms), u32(plain))
    rec = np.zeros((len(cloud), 8), F32)
    rec[:, 0:3], rec[:, 4:7] = corr[0], corr[1]
    assert np.array_equal(u32(plain), u32(grid_ref.terms29(cloud, np.arange(len(cloud), dtype=np.uint32), corr[2], rec)))
    # and a weight that is not 1 changes columns 0..26 only
    t5, w5 = R.weighted_terms29(cloud, corr, R.describe(R.CAUCHY, 0.005))
    assert (w5[corr[2]] < 1.0).any() and np.array_equal(u32(t5[:, 27:]), u32(plain[:, 27:])) and not np.array_equal(u32(t5[:, :27]), u32(plain[:, :27]))


# ---- 5. behaviour: an outlier layer pulls the plain solution, the weighted one less ---------------------------------------------------------------
def bumped_plane():
    """Scene: a bumped plane (analytic normals), 41 x 41 points over 0.2 m.  Cloud: every scene point moved by the INVERSE of a known motion M
    (1.5 degrees about (1, -2, 0.5) through the centroid, 2 mm off), so that the refinement has to find M; over a quarter of the area a planted
    layer of extra cloud points 12 mm in front of the surface (a neighbour in the pile), inside the association gate of 30 mm."""
    g = np.linspace(-0.1, 0.1, 41)
    x, y = [a.ravel() for a in np.meshgrid(g, g)]
    z = 0.6 + 0.006 * np.sin(60 * x) * np.cos(50 * y) + 0.05 * x * x
    pts = np.stack([x, y, z], 1)
    nrm = np.stack([-(0.36 * np.cos(60 * x) * np.cos(50 * y) + 0.1 * x), 0.3 * np.sin(60 * x) * np.sin(50 * y), np.ones_like(x)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ax = np.array([1.0, -2.0, 0.5]); ax /= np.linalg.norm(ax)
    th = np.deg2rad(1.5)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    M = np.eye(4)
    M[:3, :3] = Rm
    cen = pts.mean(0)
    M[:3, 3] = cen - Rm @ cen + np.array([0.002, -0.001, 0.0015])
    layer = pts[(x > 0.0) & (y > 0.0)] - np.array([0.0, 0.0, 0.012])
    inv = np.linalg.inv(M)
    cloud = np.concatenate([T.rigid_apply(inv, pts), T.rigid_apply(inv, layer)])
    return pts, nrm, cloud, len(pts), M


def weighted_float64_loop(cloud, pts, nrm, gate, iterations, kind, c):
    """truth_ref.icp's loop with the normal system weighted: columns 0..26 of every accepted correspondence times w(r), float64 throughout."""
    P = np.asarray(cloud, np.float64).copy()
    Tacc = np.eye(4)
    for _ in range(iterations):
        near = T.nearest(P, pts, gate)
        acc = near.accept
        terms, _ = T.point_to_plane_terms(P[acc], pts[near.winner[acc]], nrm[near.winner[acc]])
        if kind != R.NONE:
            r = np.einsum("ij,ij->i", pts[near.winner[acc]] - P[acc], nrm[near.winner[acc]])
            q = (r / c) ** 2
            w = {R.HUBER: np.where(np.abs(r) <= c, 1.0, c / np.maximum(np.abs(r), 1e-300)), R.TUKEY: np.where(q < 1, (1 - q) ** 2, 0.0), R.CAUCHY: 1 / (1 + q)}[kind]
            terms[:, :27] *= w[:, None]
        E, _, _ = T.float64_truth(terms.sum(0))
        P = T.rigid_apply(E, P)
        Tacc = E @ Tacc
    return Tacc


def test_weights_end_nearer_the_known_motion_than_least_squares():
    """Twelve iterations each, gate 30 mm, c = 4 mm.  Distance to the known motion: the mean displacement of the cloud's surface points between the
    found transform and M.  Observed here: start 3.06 mm, plain 2.63 mm; Huber 1.44 mm, Tukey under 0.0001 mm, Cauchy 0.49 mm (margins of 1.19,
    2.63 and 2.14 mm) -- the condition is only `nearer`."""
    pts, nrm, cloud, n_surface, M = bumped_plane()
    surface = cloud[:n_surface]

    def distance(Tm):
        return float(np.linalg.norm(T.rigid_apply(Tm, surface) - T.rigid_apply(M, surface), axis=1).mean())

    plain = distance(weighted_float64_loop(cloud, pts, nrm, 0.03, 12, R.NONE, 0.0))
    start = distance(np.eye(4))
    print(f"start {start * 1e3:.3f} mm, plain {plain * 1e3:.4f} mm")
    assert plain < start
    for kind in KINDS:
        d = distance(weighted_float64_loop(cloud, pts, nrm, 0.03, 12, kind, 0.004))
        print(f"{KIND_NAMES[kind]} {d * 1e3:.4f} mm")
        assert d < plain, (KIND_NAMES[kind], d, plain)
