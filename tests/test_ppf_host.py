"""Point-pair-feature voting, the parts that need no device: the descriptor and its tables, the model sampler's properties, the pose formula
against known rigid motions (accumulators by the numpy restatement, tests/ppf_ref.py), and every device entry point's argument checks, which
come before any device is touched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ppf_ref as R
from pose_refine_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def box_tris(sx=80.0, sy=60.0, sz=40.0):
    """A 12-triangle box, wound outwards: every face normal is exactly +-x, +-y or +-z."""
    c = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64) * [sx, sy, sz] - [sx / 2, sy / 2, sz / 2]
    f = [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)]
    return np.array([[c[i] for i in t] for t in f], np.float32)


def lump_tris():
    """The box with a smaller box standing off-centre on its top: axis-aligned normals still, but no symmetry that would make two model points
    collect the same votes."""
    return np.concatenate([box_tris(), box_tris(28.0, 18.0, 22.0) + np.array([21.0, -14.0, 31.0], np.float32)])


@pytest.fixture(scope="module")
def obj06():
    return api.Model(os.path.join(GOLDEN, "obj_06.ply"))


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------------
def test_describe_tables_against_double_cosines():
    pp = api.ppf_describe(186.0, 9.3, 15, 30)
    assert (pp.n_dist, pp.n_angle, pp.n_alpha, pp.n_keys) == (20, 15, 30, 20 * 15 ** 3)
    assert pp.dist_step == np.float32(9.3) and pp.inv_dist_step == np.float32(1.0) / np.float32(9.3)
    for k in range(16):
        assert pp.cos_edge[k] == np.float32(math.cos(k * math.pi / 15))
    for k in range(16):
        assert pp.alpha_edge[k] == np.float32(math.cos(k * 2.0 * math.pi / 30))
    for b in range(30):
        a = (b + 0.5) * 2.0 * math.pi / 30
        assert abs(pp.alpha_cos[b] - math.cos(a)) <= 2e-16 and abs(pp.alpha_sin[b] - math.sin(a)) <= 2e-16
    assert all(v == 0 for v in pp.cos_edge[16:]) and all(v == 0 for v in pp.alpha_edge[16:])
    big = api.ppf_describe(64.0, 1.0, 32, 64)                    # every cap at once
    assert big.n_dist == 64 and big.n_keys == 1 << 21


@pytest.mark.parametrize("args", [(0.0, 1.0, 15, 30), (100.0, 0.0, 15, 30), (float("nan"), 1.0, 15, 30), (100.0, float("inf"), 15, 30), (100.0, -1.0, 15, 30),
                                  (65.0, 1.0, 15, 30), (100.0, 5.0, 1, 30), (100.0, 5.0, 33, 30), (100.0, 5.0, 15, 31), (100.0, 5.0, 15, 0), (100.0, 5.0, 15, 66)])
def test_describe_refuses_and_writes_nothing(args):
    pp = _lib.PPFParams()
    C.memset(C.addressof(pp), 0xAB, C.sizeof(pp))
    before = bytes(pp)
    rc = _lib.load().pr_ppf_describe(args[0], args[1], args[2], args[3], 0, C.addressof(pp))
    assert rc == _lib.PR_ERR_INVALID and bytes(pp) == before
    assert _lib.load().pr_ppf_describe(100.0, 5.0, 15, 30, 0, None) == _lib.PR_ERR_INVALID


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
def _sampler_properties(tris, step):
    pts, nrm = api.ppf_model_sample(tris, step)
    assert 0 < len(pts) <= _lib.PPF_MAX_MODEL_POINTS
    vox = np.floor(pts.astype(np.float64) / float(np.float32(step))).astype(np.int64)
    assert len(np.unique(vox, axis=0)) == len(pts)                # no two kept points share a voxel
    # replay the definition: the first lattice point of every voxel, in (triangle, lattice) order, with its face's normal
    seen, want_p, want_t = set(), [], []
    lat = [R.lattice(t, np.float32(step)) for t in tris]
    for ti, l in enumerate(lat):
        for p, k in zip(l, np.floor(l.astype(np.float64) / float(np.float32(step))).astype(np.int64)):
            if tuple(k) not in seen:
                seen.add(tuple(k)); want_p.append(p); want_t.append(ti)
    assert np.array_equal(np.array(want_p, np.float32), pts)
    t64 = np.asarray(tris, np.float64)[want_t]
    fn = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    assert np.abs(nrm - fn).max() <= 1e-7                          # the normalised face normal, rounded
    # every point lies on its triangle within 1e-3 mm: in its plane and inside (barycentric coordinates from the lattice are >= 0 by construction)
    d = np.einsum("ij,ij->i", pts.astype(np.float64) - t64[:, 0], fn)
    assert np.abs(d).max() <= 1e-3
    b = np.linalg.lstsq(np.stack([t64[0, 1] - t64[0, 0], t64[0, 2] - t64[0, 0]], 1), pts[0].astype(np.float64) - t64[0, 0], rcond=None)[0]
    assert b.min() >= -1e-5 and b.sum() <= 1 + 1e-5
    # every lattice point (spacing <= step, so every triangle larger than a voxel has several) has a kept sample within step * sqrt(3)
    P64 = pts.astype(np.float64)
    for l in lat[::max(1, len(lat) // 200)]:
        if len(l):
            dd = np.sqrt(((l.astype(np.float64)[:, None] - P64[None]) ** 2).sum(2)).min(1)
            assert dd.max() <= float(np.float32(step)) * math.sqrt(3.0) * (1 + 1e-6)
    return pts, nrm


def test_sampler_box_and_obj06_default_step(obj06):
    for tris in (box_tris(), obj06.tris):
        pm = api.PPFModel(tris)                                    # the default step: 0.05 of the diameter
        assert len(pm.points) <= _lib.PPF_MAX_MODEL_POINTS and len(pm.points) * 30 <= _lib.PPF_MAX_CELLS
        pts, nrm = _sampler_properties(np.asarray(tris, np.float32).reshape(-1, 3, 3), pm.step_mm)
        assert np.array_equal(pts, pm.points) and np.array_equal(nrm, pm.normals)
    assert len(api.PPFModel(box_tris()).points) > 300             # a 12-triangle box is sampled densely, not at its 8 corners


def test_sampler_flip_degenerate_and_cap(obj06):
    t = box_tris()
    p0, n0 = api.ppf_model_sample(t, 7.0)
    p1, n1 = api.ppf_model_sample(t, 7.0, flip_normals=True)
    assert np.array_equal(p0, p1) and np.array_equal(n0, -n1)
    deg = np.concatenate([np.zeros((1, 3, 3), np.float32), t])     # a degenerate triangle in front changes nothing
    p2, n2 = api.ppf_model_sample(deg, 7.0)
    assert np.array_equal(p0, p2) and np.array_equal(n0, n2)
    with pytest.raises(api.PoseRefineError) as e:                   # too fine: the caller coarsens the step
        api.ppf_model_sample(obj06.tris, 1.0)
    assert e.value.code == _lib.PR_ERR_INVALID
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(api.PoseRefineError):
            api.ppf_model_sample(t, bad)


# ---- the pose formula against known rigid motions -------------------------------------------------------------------------------------------
def _rigid(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.uniform(-50, 50, 3) + [0, 0, 300]
    return T


def _axis_swap():
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                 # 90 degrees about z: scene normals stay exactly on the axes
    T[:3, 3] = [16, -32, 256]
    return T


def _rot_err(Ra, Rb):
    return math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0)))


@pytest.mark.parametrize("case", ["obj06_random", "box_random", "box_axis_swap", "box_identity"])
def test_exact_copy_votes_and_pose(case, obj06):
    """The scene is the model's sample moved by a known T (float64, rounded to float32 once), plus a copy of one reference (L == 0) and one point
    three diameters away.  For every reference chosen by hand the accumulator's peak is the right model point and its pose is T up to one alpha
    bin.  Lost votes: a pair counts for the right model point unless rounding moves one of its four features across a bin edge between model and
    scene; with coordinates up to 400 mm (float32 spacing 3e-5 mm) against pair lengths of 5 mm and more the features move by < 2e-5, the narrowest
    bin is 0.02 wide in the cosine, so at most 4 * 2 * 2e-5 / 0.02 = 0.8 % of the pairs can be lost.  Measured with this reference: 0 of 239 to 685 pairs
    in every case and reference below."""
    if case.startswith("obj06"):
        pm = api.PPFModel(obj06, step_mm=14.0)
    else:
        pm = api.PPFModel(lump_tris())
    T = {"obj06_random": _rigid(3), "box_random": _rigid(4), "box_axis_swap": _axis_swap(), "box_identity": np.eye(4)}[case]
    tb = R.tables(pm.params)
    n = len(pm.points)
    sp = (pm.points.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    sn = (pm.normals.astype(np.float64) @ T[:3, :3].T).astype(np.float32)
    refs = [0, 7, n // 2, n - 1]
    if case.startswith("box"):                                      # model normals exactly +-x, +-y, +-z: the frame's axis choice ties
        assert set(np.abs(pm.normals).max(1)) == {1.0} and len({tuple(v) for v in pm.normals}) == 6
        refs += [int(np.flatnonzero(pm.normals[:, a] == s)[0]) for a in range(3) for s in (1.0, -1.0)]
    far = sp[0] + np.float32(3 * pm.diameter)
    sp = np.concatenate([sp, sp[refs[1]][None], far[None]])
    sn = np.concatenate([sn, sn[refs[1]][None], sn[0][None]])
    offsets, ent = R.model_table(tb, pm.points, pm.normals)
    w = 2.0 * math.pi / tb["n_alpha"]
    radius = np.linalg.norm(pm.points.astype(np.float64), axis=1).max()
    for ref in refs:
        ok_m = R.pairs(tb, pm.points[ref], pm.normals[ref], pm.points, pm.normals)[0]
        acc, n_pairs = R.accumulator(tb, offsets, ent, n, sp, sn, ref)
        ok_s = R.pairs(tb, sp[ref], sn[ref], sp, sn)[0]
        assert n_pairs == ok_s.sum()
        assert not ok_s[ref] and not ok_s[-1]                       # itself (L == 0) and the point beyond the diameter are not pairs
        assert ok_s[-2] == (ref != refs[1] and ok_s[refs[1]])       # the coincident copy of refs[1]: skipped by refs[1], a pair like refs[1] for the others
        true_pairs = int(ok_m.sum())                                # what the model's table holds for this reference
        (votes, m, b), = R.peaks(acc, 1)
        if case == "box_axis_swap":
            # model and scene normals both on the axes: the frames differ by a multiple of 90 degrees, so alpha is 0 or 180 degrees for some references --
            # exactly ON a bin edge, where the rounding of the moved coordinates decides pair by pair between the two bins (votes are not spread to
            # neighbouring bins: the header's "not offered").  The right model point still collects the most votes over its bins, and either bin
            # of the edge is within one bin width of the truth.
            m, b = int(acc.sum(1).argmax()), int(acc[ref].argmax())
        assert m == ref
        lost = true_pairs - int(acc[ref, b] if case != "box_axis_swap" else acc[ref].sum())
        print(f"{case}: reference {ref}: {true_pairs} pairs, {votes} votes at the peak, {max(lost, 0)} lost")
        assert lost <= math.ceil(0.008 * true_pairs)
        if case == "box_identity":                                  # alpha == 0 exactly, sa == +-0: the upper half-plane, bin 0, nothing lost
            assert b == 0 and acc[ref, 0] >= true_pairs              # (the other bins hold the bucket mates of the true pairs: flat faces have many)
        pose = api.ppf_peak_pose(pm.params, pm.points[m], pm.normals[m], sp[ref], sn[ref], b)
        assert np.array_equal(pose, R.peak_pose(tb, pm.points[m], pm.normals[m], sp[ref], sn[ref], b))      # the float64 formula, rounded once
        P = pose.astype(np.float64)
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-6 and np.array_equal(pose[3], [0, 0, 0, 1])
        assert _rot_err(P[:3, :3], T[:3, :3]) <= w + 1e-5
        assert np.linalg.norm(P[:3, 3] - T[:3, 3]) <= 2.0 * math.sin(w / 2.0) * radius + 1e-3
        assert np.linalg.norm(P[:3, :3] @ pm.points[m].astype(np.float64) + P[:3, 3] - sp[ref]) <= 1e-3       # the reference lands on itself


def test_peak_pose_refuses():
    pp = api.ppf_describe(100.0, 5.0)
    z, x = np.zeros(3, np.float32), np.array([1, 0, 0], np.float32)
    with pytest.raises(api.PoseRefineError):
        api.ppf_peak_pose(pp, z, x, z, x, 30)                       # alpha_bin == n_alpha
    with pytest.raises(api.PoseRefineError):
        api.ppf_peak_pose(pp, z, z, z, x, 0)                        # a zero normal has no frame
    assert np.array_equal(api.ppf_peak_pose(pp, z, x, z, x, 0)[3], [0, 0, 0, 1])


# ---- the device entry points check their arguments before any device is touched ------------------------------------------------------------------
FAKE = 0x10000                                                      # a non-null "device pointer": never dereferenced, the checks come first


def _vote(pp, **kw):
    a = dict(offsets=FAKE, entries=FAKE, mp=FAKE, mn=FAKE, n_model=100, sp=FAKE, sn=FAKE, n_scene=500, ref_first=0, ref_stride=1, n_refs=8, n_peaks=1,
             peaks=FAKE, poses=FAKE)
    a.update(kw)
    return _lib.load().pr_ppf_vote(C.addressof(pp) if pp is not None else None, a["offsets"], a["entries"], a["mp"], a["mn"], a["n_model"], a["sp"], a["sn"],
                                   a["n_scene"], a["ref_first"], a["ref_stride"], a["n_refs"], a["n_peaks"], a["peaks"], a["poses"], None)


def test_vote_checks_come_before_the_device():
    pp = api.ppf_describe(100.0, 5.0, 15, 30)
    bad = [dict(n_model=0), dict(n_model=2049), dict(n_model=1093), dict(n_scene=0), dict(n_scene=16385), dict(n_peaks=0), dict(n_peaks=5),
           dict(ref_stride=0), dict(ref_first=500), dict(ref_first=600), dict(ref_first=493, n_refs=8), dict(ref_stride=100, n_refs=6),
           dict(offsets=None), dict(entries=None), dict(mp=None), dict(mn=None), dict(sp=None), dict(sn=None), dict(peaks=None), dict(poses=None)]
    for kw in bad:
        assert _vote(pp, **kw) == _lib.PR_ERR_INVALID, kw
    assert _vote(None) == _lib.PR_ERR_INVALID
    odd = api.ppf_describe(100.0, 5.0, 15, 30)
    odd.n_alpha = 29
    assert _vote(odd) == _lib.PR_ERR_INVALID
    for field, value in (("n_keys", 7), ("inv_dist_step", 0.5), ("n_dist", 65), ("n_angle", 1), ("dist_step", float("nan"))):
        q = api.ppf_describe(100.0, 5.0, 15, 30)
        setattr(q, field, value)
        assert _vote(q) == _lib.PR_ERR_INVALID, field
    assert _vote(pp, n_refs=0, peaks=None, poses=None) == _lib.PR_OK                     # nothing to do: no device needed


def test_build_and_scene_checks_come_before_the_device():
    lib = _lib.load()
    pp = api.ppf_describe(100.0, 5.0, 15, 30)
    n = C.c_uint32(0)
    build = lambda params, pts, nrm, nm, off, ent, out: lib.pr_ppf_model_build_dev(params, pts, nrm, nm, off, ent, out)
    P = C.addressof(pp)
    for args in [(None, FAKE, FAKE, 10, FAKE, FAKE, C.byref(n)), (P, None, FAKE, 10, FAKE, FAKE, C.byref(n)), (P, FAKE, None, 10, FAKE, FAKE, C.byref(n)),
                 (P, FAKE, FAKE, 0, FAKE, FAKE, C.byref(n)), (P, FAKE, FAKE, 2049, FAKE, FAKE, C.byref(n)), (P, FAKE, FAKE, 10, None, FAKE, C.byref(n)),
                 (P, FAKE, FAKE, 10, FAKE, None, C.byref(n)), (P, FAKE, FAKE, 10, FAKE, FAKE, None)]:
        assert build(*args) == _lib.PR_ERR_INVALID, args
    odd = api.ppf_describe(100.0, 5.0, 15, 30)
    odd.n_alpha = 31
    assert build(C.addressof(odd), FAKE, FAKE, 10, FAKE, FAKE, C.byref(n)) == _lib.PR_ERR_INVALID
    K = (C.c_float * 9)(500, 0, 32, 0, 500, 24, 0, 0, 1)
    good = _lib.SceneProjDesc(64, 48, 0.1, K, FAKE, FAKE)
    for desc, stride, pts, nrm, out in [(None, 1, FAKE, FAKE, C.byref(n)), (good, 0, FAKE, FAKE, C.byref(n)), (good, 257, FAKE, FAKE, C.byref(n)),
                                        (good, 1, None, FAKE, C.byref(n)), (good, 1, FAKE, None, C.byref(n)), (good, 1, FAKE, FAKE, None),
                                        (_lib.SceneProjDesc(64, 48, 0.1, K, None, FAKE), 1, FAKE, FAKE, C.byref(n)),
                                        (_lib.SceneProjDesc(64, 48, 0.1, K, FAKE, None), 1, FAKE, FAKE, C.byref(n)),
                                        (_lib.SceneProjDesc(0, 48, 0.1, K, FAKE, FAKE), 1, FAKE, FAKE, C.byref(n)),
                                        (_lib.SceneProjDesc(9000, 48, 0.1, K, FAKE, FAKE), 1, FAKE, FAKE, C.byref(n))]:
        assert lib.pr_ppf_scene_points_dev(C.addressof(desc) if desc is not None else None, stride, pts, nrm, out) == _lib.PR_ERR_INVALID
