"""Support planes on the host (no GPU): the numpy reference against float64 truth, pr_plane_from_moments against what an eigenpair must satisfy,
pr_scene_planes_host against the reference byte for byte, pr_plane_describe's refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import planes_cases as PC
import planes_ref as R
from pose_refine_amd import _lib, api

F = np.float32
PARAMS = dict(stride=1, cand_stride=3, tau_mm=2.0, label_tau_mm=3.0, cos_min=0.9, min_support=100)


def prepare(depth, K=PC.K64):
    h, w = depth.shape
    pcd, nrm = np.zeros((w * h, 3), F), np.zeros((w * h, 3), F)
    d = np.ascontiguousarray(depth)
    _lib.check(_lib.load().pr_scene_proj_prepare(_lib.ptr(d), int(d.dtype == np.int32), _lib.ptr(np.asarray(K, F)), w, h, _lib.ptr(pcd), _lib.ptr(nrm)))
    return pcd, nrm


CASES = {"tilted": PC.one_plane, "edge": PC.two_planes, "box": PC.plane_with_box}


@pytest.fixture(scope="module")
def analytic():
    out = {}
    for name, make in CASES.items():
        c = make()
        c["pcd"], c["nrm"] = prepare(c["depth"])
        c["n_planes"] = 1 if name == "box" else len(c["truth"]) + 1      # (the box's top is a plane too: one plane asked for, the box keeps label 0)
        c["ref"] = R.scene_planes(c["pcd"], c["nrm"], c["depth"], PC.W, PC.H, n_planes=c["n_planes"], drop_behind=(name == "box"), **PARAMS)
        out[name] = c
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_recovers_analytic_planes(analytic, name):
    """The reference's planes against the float64 planes the frame was rendered from, within planes_cases.fit_bound's limits (derived there, not tuned)."""
    c = analytic[name]
    ref, owner, truth = c["ref"], c["owner"].reshape(-1), c["truth"]
    assert len(ref["planes"]) == len(truth)                       # an extra round, where one is asked for, finds nothing
    pts, nm, pix = R.sample(c["pcd"], c["nrm"], PC.W, PC.H, 1)
    alive = np.ones(len(pts), bool)
    labels = ref["labels"].reshape(-1)
    pmm = c["pcd"].astype(np.float64) * 1000.0
    seen = set()
    for k, pl in enumerate(ref["planes"], 1):
        inl = R.inliers(pts, nm, alive, pl["candidate"] * PARAMS["cand_stride"], PARAMS["tau_mm"], PARAMS["cos_min"])
        assert int(inl.sum()) == pl["support"]
        ids = set(owner[pix[inl]].tolist())
        assert len(ids) == 1 and 0 not in ids                     # the bound's premise: the inliers are samples of ONE analytic plane
        t = ids.pop()
        seen.add(t)
        n, d = truth[t - 1]
        p = pts[inl].astype(np.float64)
        delta, tan_theta, off_bound = PC.fit_bound(p, n, d, c["K"], PC.W, PC.H)
        assert np.abs(p @ n - d).max() <= delta                    # ... each within delta of it
        nf = pl["normal"].astype(np.float64)
        cosang = float(nf @ n)
        tan_fit = math.sqrt(max(0.0, 1.0 - cosang * cosang)) / cosang
        print(f"{name} plane {k}: tan(angle) {tan_fit:.3e} (bound {tan_theta:.3e}), offset error {abs(float(pl['offset_mm']) - d):.4f} mm (bound {off_bound:.4f})")
        assert cosang > 0 and tan_fit <= tan_theta
        assert abs(float(pl["offset_mm"]) - d) <= off_bound
        # the label sits on the right side: a pixel labelled k is as near the analytic plane as label_tau and the fit's error allow, and most of
        # the plane's own pixels carry it
        lab = labels == k
        dist = np.abs(pmm[lab] @ n - d)
        assert (dist <= PARAMS["label_tau_mm"] + off_bound + tan_theta * np.linalg.norm(pmm[lab], axis=1)).all()
        assert (labels[owner == t] == k).mean() > 0.5
        alive = ~np.isin(labels[pix], np.arange(1, k + 1)) & (labels[pix] != R.BEHIND)      # what round k + 1 ran over
    assert seen == set(range(1, len(truth) + 1))
    if name == "edge":
        assert set(np.unique(labels)) == {1, 2} | ({0} if (labels == 0).any() else set())
    if name == "box":
        assert (labels[owner == 0] == 0).all() and (ref["depth"].reshape(-1)[owner == 0] == c["depth"].reshape(-1)[owner == 0]).all()
        assert (ref["depth"].reshape(-1)[labels == 1] == 0).all() and (labels == 1).sum() > 1000


def _cloud_moments(rng, kind):
    if kind == "planar":
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        p = rng.uniform(-300, 300, (400, 3))
        p -= np.outer(p @ n - 500.0, n)
        p += rng.normal(scale=0.3, size=p.shape)
    elif kind == "blob":
        p = rng.normal(scale=[50.0, 20.0, 5.0], size=(300, 3)) + [10.0, -20.0, 700.0]
    elif kind == "far":
        p = rng.uniform(-2000, 2000, (65536, 3)); p[:, 2] = 60000.0 + rng.normal(scale=0.5, size=len(p))
    elif kind == "through_origin":                                  # symmetric about the origin in the plane z = 0: the sums vanish, offset == 0
        q = rng.uniform(-100, 100, (50, 2))
        p = np.concatenate([np.c_[q, np.zeros(50)], np.c_[-q, np.zeros(50)]])
    elif kind == "through_origin_x":                                # the plane x = 0: the first non-zero component is x
        q = rng.uniform(-100, 100, (50, 2))
        p = np.concatenate([np.c_[np.zeros(50), q], np.c_[np.zeros(50), -q]])
    elif kind == "three":
        p = np.array([[0.0, 0.0, 500.0], [100.0, 0.0, 510.0], [0.0, 100.0, 490.0]])
    return R.moments_of(p.astype(F))


@pytest.mark.parametrize("kind", ["planar", "blob", "far", "through_origin", "through_origin_x", "three"])
def test_from_moments_is_an_eigenpair(kind):
    rng = np.random.default_rng(3)
    for _ in range(1 if kind in ("three", "far") else 8):
        m = _cloud_moments(rng, kind)
        nrm, off, rms, eig = api.plane_from_moments(m)
        Cm = np.array(R.scatter(m), dtype=object).astype(np.float64)
        assert np.linalg.norm(Cm @ nrm - eig[0] * nrm) <= 1e-12 * np.linalg.norm(Cm)
        assert eig[0] <= eig[1] and eig[0] <= eig[2]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 4e-16
        want_off = float(nrm @ m[1:4].astype(np.float64)) / float(m[0]) / 16.0
        assert off <= 0.0 and abs(off - want_off) <= 1e-12 * max(1.0, abs(want_off))
        if kind.startswith("through_origin"):
            assert off == 0.0 and nrm[np.flatnonzero(nrm)[0]] < 0.0
            assert abs(nrm[2 if kind == "through_origin" else 0]) > 0.999999
        ref_n, ref_off, ref_rms, ref_eig = R.from_moments(m)        # and the reference's refit, bit for bit
        assert nrm.tobytes() == np.array(ref_n).tobytes() and off == ref_off and rms == ref_rms and eig.tobytes() == np.array(ref_eig).tobytes()


def test_from_moments_refusals():
    two = R.moments_of(np.array([[0, 0, 500], [10, 0, 500]], F))
    point = R.moments_of(np.tile(np.array([[12.5, -3.25, 640.0]], F), (7, 1)))          # collinear down to a point: the scatter matrix is all zero
    for m in (two, point):
        with pytest.raises(api.PoseRefineError) as e:
            api.plane_from_moments(m)
        assert e.value.code == _lib.PR_ERR_INVALID
        with pytest.raises(R.Invalid):
            R.from_moments(m)
    assert _lib.load().pr_plane_from_moments(None, None, None, None, None) == _lib.PR_ERR_INVALID


@pytest.fixture(scope="module")
def synthetic_refs():
    out = {}
    for name, fkw, pkw in PC.synthetic_variants():
        pcd, nrm, depth, facts = PC.synthetic(**fkw)
        out[name] = (pcd, nrm, depth, pkw, R.scene_planes(pcd, nrm, depth, PC.W, PC.H, **pkw))
    return out


@pytest.mark.parametrize("name", [v[0] for v in PC.synthetic_variants()])
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_host_equals_reference_synthetic(synthetic_refs, name, dtype):
    pcd, nrm, depth, pkw, ref = synthetic_refs[name]
    ref = dict(ref, depth=ref["depth"].astype(dtype))
    got = api.scene_planes_host(pcd, nrm, depth.astype(dtype), PC.W, PC.H, want_moments=True, want_supports=True, **pkw)
    PC.assert_same(got, ref, pkw["n_planes"])
    if name == "stride1_edges":                                    # what the frame was built to hit
        facts = PC.synthetic()[3]
        assert len(ref["planes"]) == 2 and pkw["n_planes"] == 3    # the third round fails min_support
        lab = ref["labels"]
        r0 = facts["row_a"]
        pts, nm, pix = R.sample(pcd, nrm, PC.W, PC.H, 1)
        c0, c12, c24, c36, c48, c60 = (int(np.flatnonzero(pix == r0 * PC.W + x)[0]) for x in (0, 12, 24, 36, 48, 60))
        sup = ref["supports"][0]
        assert c12 < c24 and sup[c12] == sup[c24] == sup.max() and ref["planes"][0]["candidate"] == c12      # the tie: the lower index wins
        everyone = np.ones(len(pts), bool)
        in0 = R.inliers(pts, nm, everyone, c0, pkw["tau_mm"], pkw["cos_min"])                                  # a plain candidate of plane A against the planted edges
        assert abs(float(pts[c12][2] - pts[c0][2])) == pkw["tau_mm"] and in0[c12] and in0[c24] and not in0[c36]
        assert float(R.dot(nm[c0][0], nm[c0][1], nm[c0][2], nm[c48][0], nm[c48][1], nm[c48][2])) == pkw["cos_min"] and in0[c48] and not in0[c60]
        assert lab[1, 2] == R.NO_DEPTH and not (lab == R.BEHIND).any() and ref["supports"][2].any()
    if name == "stride3":                                          # plane B lies behind plane A: dropped with everything else there, one plane found
        assert len(ref["planes"]) == 1 and ref["planes"][0]["behind"] == (ref["labels"] == R.BEHIND).sum() > 100
    if name == "one_plane_three_asked":
        assert len(ref["planes"]) == 1 and not (ref["labels"] == R.BEHIND).any()
    if name == "stride4_one_candidate":
        assert ref["n_candidates"] == 1


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_reference_analytic(analytic, name):
    c = analytic[name]
    n_planes = c["n_planes"]
    got = api.scene_planes_host(c["pcd"], c["nrm"], c["depth"], PC.W, PC.H, n_planes=n_planes, drop_behind=(name == "box"), want_moments=True, want_supports=True, **PARAMS)
    PC.assert_same(got, c["ref"], n_planes)


def test_host_empty_sample_and_caps():
    pcd, nrm, depth, _ = PC.synthetic()
    none = np.zeros_like(nrm)
    planes, labels, cleared = api.scene_planes_host(pcd, none, depth, PC.W, PC.H, stride=1, min_support=3)
    assert len(planes) == 0 and np.array_equal(labels == 0, pcd[..., 2] > 0) and np.array_equal(labels == R.NO_DEPTH, pcd[..., 2] <= 0)
    assert np.array_equal(cleared, depth)
    w, h = 320, 240                                                 # 76 800 samples at stride 1: over PLANE_MAX_SAMPLES
    big_p, big_n = np.ones((w * h, 3), F), np.ones((w * h, 3), F)
    with pytest.raises(api.PoseRefineError) as e:
        api.scene_planes_host(big_p, big_n, np.ones((h, w), np.uint16), w, h, stride=1)
    assert e.value.code == _lib.PR_ERR_INVALID
    with pytest.raises(api.PoseRefineError) as e:                   # 19 200 samples, every one a candidate: over PLANE_MAX_CANDIDATES
        api.scene_planes_host(big_p, big_n, np.ones((h, w), np.uint16), w, h, stride=2, cand_stride=1)
    assert e.value.code == _lib.PR_ERR_INVALID
    with pytest.raises(R.Invalid):
        R.scene_planes(big_p, big_n, np.ones((h, w), np.uint16), w, h, stride=1)


@pytest.mark.parametrize("bad", [dict(stride=0), dict(stride=257), dict(cand_stride=0), dict(tau_mm=-1.0), dict(tau_mm=float("nan")), dict(tau_mm=float("inf")),
                                 dict(label_tau_mm=-0.5), dict(label_tau_mm=float("inf")), dict(cos_min=1.5), dict(cos_min=-1.5), dict(cos_min=float("nan")),
                                 dict(min_support=2), dict(n_planes=0), dict(n_planes=5)])
def test_describe_refusals(bad):
    with pytest.raises(api.PoseRefineError) as e:
        api.PlaneParams(**bad)
    assert e.value.code == _lib.PR_ERR_INVALID


def test_describe_fills_and_null_out():
    pp = api.PlaneParams(stride=3, cand_stride=5, tau_mm=1.5, label_tau_mm=2.5, cos_min=-2.0, min_support=7, n_planes=4, drop_behind=False)
    assert (pp.stride, pp.cand_stride, pp.tau_mm, pp.label_tau_mm, pp.cos_min, pp.min_support, pp.n_planes, pp.drop_behind) == (3, 5, 1.5, 2.5, -2.0, 7, 4, 0)
    assert _lib.load().pr_plane_describe(4, 16, 3.0, 6.0, 0.9, 500, 1, 1, None) == _lib.PR_ERR_INVALID
    bad = _lib.PlaneParamsDesc(4, 16, 3.0, 6.0, 0.9, 500, 9, 1)     # a block that pr_plane_describe would not have filled is refused by the entry points
    n = C.c_uint32(0)
    z = np.zeros(16, np.uint8)
    assert _lib.load().pr_scene_planes_host(_lib.ptr(z), _lib.ptr(z), None, 0, 1, 1, C.addressof(bad), _lib.ptr(z), None, _lib.ptr(z), None, None, C.byref(n)) == _lib.PR_ERR_INVALID
