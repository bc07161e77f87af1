"""Host side of contour alignment (no GPU): the record layout, the argument errors of the entry points before any device is touched, the
reference nearest map by two formulations, pr_info_eig / pr_info_combine / pr_info_step against tests/contour_fit_ref.py, and the plate-on-wall
case through the reference loop over oracle renders: the surface leaves three motions free, the silhouette pins them, eight steps bring the
plate back."""
import ctypes as C
import math

import numpy as np
import pytest

import contour_fit_ref as CF
import info_ref as I
import oracle_lib as O
from contour_ref import NO_EDGE, edge_distance_ref, edges
from pose_refine_amd import _lib, api
from test_information_host import records_of

F32, F64 = np.float32, np.float64
NO_ROI = _lib.Roi(0, 0, 0, 0)


class ContourFit(C.Structure):
    """pr_contour_fit as the header declares it."""
    _fields_ = [("contour", C.c_uint32), ("used", C.c_uint32), ("occluded", C.c_uint32), ("miss", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("sum_d2", C.c_uint64)]


def test_record_layout_and_abi_version():
    assert C.sizeof(ContourFit) == 32 and api.CONTOUR_FIT.itemsize == 32 and _lib.CONTOUR_FIT is api.CONTOUR_FIT
    for name, _ in ContourFit._fields_:
        assert api.CONTOUR_FIT.fields[name][1] == getattr(ContourFit, name).offset, name
    assert [api.CONTOUR_FIT.fields[f][1] for f in ("contour", "used", "occluded", "miss", "reserved", "sum_d2")] == [0, 4, 8, 12, 16, 24]
    assert [api.CONTOUR.fields[f][1] for f in ("contour", "hit", "occluded", "miss", "reserved", "dist_sum")] == [0, 4, 8, 12, 16, 24]
    assert api.EDGE_NONE == 0xFFFFFFFF == CF.NONE
    assert _lib.POSE_INFO.itemsize == 272                            # the struct is unchanged ...
    assert _lib.load().pr_abi_version() == 4                         # ... and so is the ABI


# ---- argument errors, before any device is touched ---------------------------------------------------------------------------------------------
def _contour_information_args():
    """A complete, valid argument list of pr_contour_information (the device pointers are never followed: every refusal comes first)."""
    keep = dict(poses=np.tile(np.eye(4, dtype=F32), (2, 1, 1)), proj=np.eye(4, dtype=F32), K=np.array([200, 0, 32, 0, 200, 24, 0, 0, 1], F32),
                cm=np.zeros(3, F32), sc=np.zeros(2, api.SCORE), fit=np.zeros(2, api.CONTOUR_FIT), info=np.zeros(2, _lib.POSE_INFO))
    fake = 0x1000                                                    # stands for device memory
    args = dict(tris=fake, n_tris=1, poses=_lib.ptr(keep["poses"]), n=2, W=64, H=48, proj=_lib.ptr(keep["proj"]), roi=NO_ROI, scene=fake, i32=1, tau=5, jump=10,
                nearest=fake, K=_lib.ptr(keep["K"]), cm=_lib.ptr(keep["cm"]), radius=0.1, sc=_lib.ptr(keep["sc"]), fit=_lib.ptr(keep["fit"]),
                info=_lib.ptr(keep["info"]))
    return args, keep


def test_contour_information_argument_errors():
    lib = _lib.load()
    args, keep = _contour_information_args()
    nan, inf = float("nan"), float("inf")
    bad_K = [keep["K"].copy() for _ in range(3)]
    bad_K[0][0], bad_K[1][4], bad_K[2][2] = 0.0, 0.0, nan
    bad_c = np.array([0.0, inf, 0.0], F32)
    bad_pose = keep["poses"].copy()
    bad_pose[1, 0, 3] = nan
    cases = [dict(tau=-1), dict(jump=-1), dict(nearest=None), dict(fit=None), dict(info=None), dict(K=None), dict(cm=None), dict(scene=None), dict(proj=None),
             dict(poses=None), dict(tris=None), dict(W=0), dict(H=0), dict(W=8193), dict(roi=_lib.Roi(60, 0, 10, 10)), dict(radius=0.0), dict(radius=-1.0),
             dict(radius=nan), dict(radius=inf), dict(cm=_lib.ptr(bad_c)), dict(poses=_lib.ptr(bad_pose))] + [dict(K=_lib.ptr(k)) for k in bad_K]
    for kw in cases:
        a = dict(args, **kw)
        assert lib.pr_contour_information(*a.values()) == _lib.PR_ERR_INVALID, kw
    for f in ("sc", "fit", "info"):
        assert not keep[f].tobytes().strip(b"\0"), f                # nothing written
    assert b"pr_contour_information" in lib.pr_last_error()
    # no hypotheses: PR_OK with null arrays, nothing touched; the intrinsics and the centre are checked all the same
    none = dict(args, n=0, poses=None, sc=None, fit=None, info=None, tris=None, scene=None, nearest=None)
    assert lib.pr_contour_information(*none.values()) == _lib.PR_OK
    assert lib.pr_contour_information(*dict(none, K=None).values()) == _lib.PR_ERR_INVALID
    # the mesh table of a mixed batch
    table = (_lib.MeshRef * 2)(_lib.MeshRef(0x1000, 1), _lib.MeshRef(0x2000, 1))
    idx, cms, rad = np.array([0, 1], np.uint32), np.zeros((2, 3), F32), np.array([0.1, 0.2], F32)

    def multi(**kw):
        a = dict(meshes=table, n_meshes=2, idx=_lib.ptr(idx), poses=args["poses"], n=2, W=64, H=48, proj=args["proj"], roi=NO_ROI, scene=0x1000, i32=1, tau=5,
                 jump=10, nearest=0x1000, K=args["K"], cms=_lib.ptr(cms), rad=_lib.ptr(rad), sc=None, fit=args["fit"], info=args["info"])
        a.update(kw)
        return lib.pr_contour_information_multi(*a.values())
    bad_idx, bad_rad = np.array([0, 2], np.uint32), np.array([0.1, 0.0], F32)
    for kw in (dict(idx=_lib.ptr(bad_idx)), dict(rad=_lib.ptr(bad_rad)), dict(rad=None), dict(cms=None), dict(idx=None), dict(meshes=None), dict(jump=-1),
               dict(nearest=None), dict(fit=None), dict(info=None), dict(K=None)):
        assert multi(**kw) == _lib.PR_ERR_INVALID, kw
    assert b"pr_contour_information_multi" in lib.pr_last_error()
    assert multi(n=0) == _lib.PR_OK
    with pytest.raises(ValueError):
        api.contour_information(np.zeros((1, 3, 3), F32), np.eye(4, dtype=F32)[None], 64, 48, np.eye(4), keep["K"], np.zeros((48, 64), np.int32), 5, 10,
                                None)                                # center and radius default only for a Model


def test_device_calls_without_gpu_fail_loudly():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is covered on the CPU-only box")
    lib = _lib.load()
    assert lib.pr_scene_edge_nearest_dev(None, 1, 64, 48, 10, 3, None) == _lib.PR_ERR_NO_DEVICE
    args, _ = _contour_information_args()
    assert lib.pr_contour_information(*args.values()) == _lib.PR_ERR_NO_DEVICE
    with pytest.raises(api.PoseRefineError) as e:
        api.scene_edge_nearest(np.zeros((48, 64), np.int32), 64, 48, 10, 3)
    assert e.value.code == _lib.PR_ERR_NO_DEVICE


# ---- the reference nearest map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (33, 1), (23, 31), (40, 70)])
@pytest.mark.parametrize("radius", [0, 1, 3, 32])
def test_reference_nearest_by_two_formulations(shape, radius):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + radius)
    for density in (0.0, 0.002, 0.03, 0.5):
        e = rng.random(shape) < density
        N = CF.nearest_separable(e, radius)
        assert N.dtype == np.uint32 and np.array_equal(N, CF.nearest_brute(e, radius)), (shape, radius, density)
        ys, xs = np.nonzero(e)
        assert np.array_equal(N[ys, xs], (ys << 16) | xs)           # an edge pixel is its own nearest
        if not e.any():
            assert (N == CF.NONE).all()


def test_reference_nearest_ties_by_hand():
    e = np.zeros((5, 5), bool)
    e[2, 0] = e[2, 4] = e[0, 2] = e[4, 2] = True                     # four edge pixels at distance 2 of the centre
    N = CF.nearest_brute(e, 2)
    assert N[2, 2] == (0 << 16) | 2                                  # the smaller ey
    e[0, 2] = False
    assert CF.nearest_brute(e, 2)[2, 2] == (2 << 16) | 0            # then the smaller ex within the row ...
    assert CF.nearest_separable(e, 2)[2, 2] == (2 << 16) | 0
    e[1, 1] = True                                                   # ... but the smaller squared distance first: (1, 1) at 2 against 4
    assert CF.nearest_brute(e, 2)[2, 2] == (1 << 16) | 1 == CF.nearest_separable(e, 2)[2, 2]
    assert CF.nearest_brute(e, 1)[2, 2] == (1 << 16) | 1 and CF.nearest_brute(e, 0)[2, 2] == CF.NONE


@pytest.mark.parametrize("radius", [0, 1, 3, 32])
def test_nearest_exists_exactly_where_the_distance_does(scenario, radius):
    from contour_ref import structured_scene
    sc = structured_scene(scenario["depth"][1])[100:260, 150:420]
    for jump in (0, 10):
        N, D = CF.nearest_ref(sc, jump, radius), edge_distance_ref(sc, jump, radius)
        assert np.array_equal(N != CF.NONE, D != NO_EDGE)
        ys, xs = np.nonzero(N != CF.NONE)
        ey, ex = (N[ys, xs] >> 16).astype(np.int64), (N[ys, xs] & 0xFFFF).astype(np.int64)
        assert edges(sc, jump)[ey, ex].all()
        cheb = np.maximum(np.abs(ey - ys), np.abs(ex - xs))
        assert (cheb <= radius).all() and (cheb >= D[ys, xs]).all()  # inside the window; never nearer than the chessboard distance says


# ---- pr_info_eig ---------------------------------------------------------------------------------------------------------------------------------
def _eig_holds(info, eig, what):
    Hm, lam, V = I.sym6(info["H"]), np.asarray(eig["lambda"], F64), np.asarray(eig["V"], F64).reshape(6, 6)
    top = max(lam[5], 0.0)
    assert float(np.abs(Hm @ V - V * lam[None, :]).max()) <= 1e-12 * top, what
    assert float(np.abs(V.T @ V - np.eye(6)).max()) <= 1e-12, what
    assert (np.diff(lam) >= 0).all() and int(eig["sweeps"]) <= _lib.INFO_MAX_SWEEPS and int(eig["reserved"]) == 0, what
    for k in range(6):
        assert V[int(np.argmax(np.abs(V[:, k]))), k] > 0, (what, k)


@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_info_eig_on_analytic_records(name):
    info, _, dim = records_of(name)
    eig = api.information_eig(info)
    _eig_holds(info, eig[0], name)
    lam, V, sweeps = CF.jacobi(np.asarray(info["H"]).reshape(21))
    assert int(eig[0]["sweeps"]) == sweeps > 0
    assert np.abs(eig[0]["lambda"] - lam).max() <= 1e-12 * lam[5] and np.abs(np.asarray(eig[0]["V"]).reshape(6, 6) @ np.diag(lam) @ np.asarray(eig[0]["V"]).reshape(6, 6).T
                                                                             - V @ np.diag(lam) @ V.T).max() <= 1e-12 * lam[5]
    assert I.rank_of(eig[0]["lambda"], 1e-6) == 6 - dim == 3       # three free motions each


def test_info_eig_diagonal_and_zero():
    info = np.zeros(2, _lib.POSE_INFO)
    diag = [5.0, 1.0, 3.0, 0.0, 2.0, 4.0]
    H = np.zeros(21)
    H[[0, 6, 11, 15, 18, 20]] = diag
    info["H"][0] = H
    eig = api.information_eig(info)
    assert eig["sweeps"].tolist() == [0, 0]
    assert eig[0]["lambda"].tolist() == sorted(diag) and not eig[1]["lambda"].any()
    V = np.asarray(eig[0]["V"]).reshape(6, 6)
    assert np.array_equal(V[:, np.argsort(np.argsort(diag))], np.eye(6))      # a permutation of the axes, every sign positive
    assert np.array_equal(np.asarray(eig[1]["V"]).reshape(6, 6), np.eye(6))
    _eig_holds(info[0], eig[0], "diagonal")
    lib = _lib.load()
    assert lib.pr_info_eig(None, _lib.ptr(eig)) == _lib.PR_ERR_INVALID and lib.pr_info_eig(_lib.ptr(info), None) == _lib.PR_ERR_INVALID


# ---- pr_info_combine, pr_info_step ---------------------------------------------------------------------------------------------------------------
def _random_info(seed, c=(0.01, -0.02, 0.9), rho=0.1, rank=6):
    g = np.random.default_rng(seed)
    J = g.normal(size=(40, 6))
    J[:, rank:] = 0.0
    r = g.normal(size=40) * 1e-3
    o = np.zeros(1, _lib.POSE_INFO)[0]
    Hm = J.T @ J
    o["H"], o["g"] = Hm[np.triu_indices(6)], J.T @ r
    o["c"], o["rho"], o["n_points"], o["n_valid"], o["n_zero_weight"] = np.asarray(c, F32), F32(rho), 50 + seed, 40, seed
    o["sum_w"], o["sum_wr2"], o["sum_r2"] = 40.0, float(r @ r), float(r @ r) * 2
    return o


def test_info_combine_follows_the_reference():
    a, b = _random_info(1), _random_info(2)
    for wa, wb in ((1.0, 1.0), (1.0, 0.25), (0.0, 3.0), (2.5, 0.0)):
        got, want = api.combine_information(a, b, wa, wb)[0], CF.combine(a, wa, b, wb)
        assert got.tobytes() == want.tobytes(), (wa, wb)
    assert api.combine_information(a, b, 1.0, 0.0)[0]["H"].tolist() == a["H"].tolist()
    lib = _lib.load()
    out = np.zeros(1, _lib.POSE_INFO)
    pa, pb = _lib.ptr(np.array([a])), _lib.ptr(np.array([b]))
    other_c, other_rho = np.array([_random_info(2, c=(0.01, -0.02, 0.9000001))]), np.array([_random_info(2, rho=0.2)])
    A, B = np.array([a]), np.array([b])
    for args in ((None, 1.0, _lib.ptr(B), 1.0, _lib.ptr(out)), (_lib.ptr(A), 1.0, None, 1.0, _lib.ptr(out)), (_lib.ptr(A), 1.0, _lib.ptr(B), 1.0, None),
                 (_lib.ptr(A), -1.0, _lib.ptr(B), 1.0, _lib.ptr(out)), (_lib.ptr(A), 1.0, _lib.ptr(B), float("nan"), _lib.ptr(out)),
                 (_lib.ptr(A), float("inf"), _lib.ptr(B), 1.0, _lib.ptr(out)), (_lib.ptr(A), 1.0, _lib.ptr(other_c), 1.0, _lib.ptr(out)),
                 (_lib.ptr(A), 1.0, _lib.ptr(other_rho), 1.0, _lib.ptr(out))):
        assert lib.pr_info_combine(*args) == _lib.PR_ERR_INVALID, args
    assert not out.tobytes().strip(b"\0")                            # nothing written
    del pa, pb


def _pose(seed):
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    p = np.eye(4)
    p[:3, :3] = q * np.sign(np.linalg.det(q))
    p[:3, 3] = [12.0, -20.0, 900.0]
    return p.astype(F32)


def test_info_step_follows_the_reference():
    for seed, rank in ((3, 6), (4, 6), (5, 4), (6, 1)):
        info = _random_info(seed, rank=rank)
        eig = api.information_eig(info)[0]
        pose = _pose(seed)
        got, delta, r = api.information_step(info, eig, pose[None], 1e-9)
        want, wdelta, wrank = CF.step(info["g"], info["c"], info["rho"], eig["lambda"], eig["V"], 1e-9, pose)
        assert int(r[0]) == wrank == rank
        assert np.abs(delta[0] - wdelta).max() <= 1e-12 * np.abs(wdelta).max()
        assert np.abs(got[0].astype(F64) - want.astype(F64)).max() <= 2.0 ** -23 * 1000.0      # one float32 ulp of the largest entry (below 1024 mm)
        assert np.array_equal(got[0][3], pose[3])
        # delta solves the system on the kept subspace, and has no component outside it
        V, lam = np.asarray(eig["V"]).reshape(6, 6), np.asarray(eig["lambda"])
        kept = V[:, 6 - rank:]
        assert np.abs(kept.T @ (I.sym6(info["H"]) @ delta[0] - info["g"])).max() <= 1e-9 * np.abs(info["g"]).max()
        if rank < 6:
            assert np.abs(V[:, :6 - rank].T @ delta[0]).max() <= 1e-15 * np.abs(delta[0]).max() + 1e-300


def test_info_step_pure_rotation_about_c_leaves_c_fixed():
    """g along a rotational axis only, H = I: delta = g, a rotation by |g| / rho about c -- the camera-frame point c (metres) stays where it is."""
    info = np.zeros(1, _lib.POSE_INFO)[0]
    info["H"] = np.eye(6)[np.triu_indices(6)]
    info["g"] = [0.02, -0.01, 0.03, 0.0, 0.0, 0.0]
    info["c"], info["rho"] = F32([0.05, -0.03, 0.9]), F32(0.1)
    eig = api.information_eig(info)[0]
    pose = np.eye(4, dtype=F32)
    pose[:3, 3] = np.asarray(info["c"], F64) * 1000.0                # the model origin sits at c
    got, delta, rank = api.information_step(info, eig, pose[None], 0.0)
    assert rank[0] == 6 and np.allclose(delta[0], info["g"], rtol=0, atol=1e-17)
    assert np.abs(got[0][:3, 3].astype(F64) - pose[:3, 3]).max() <= 2.0 ** -23 * 1024.0       # c fixed, to float32 rounding of millimetres
    angle = math.acos((np.trace(got[0][:3, :3].astype(F64)) - 1.0) / 2.0)
    assert abs(angle - np.linalg.norm(info["g"][:3]) / 0.1) <= 1e-6
    assert np.allclose(got[0][:3, :3].astype(F64), CF.rodrigues(np.asarray(info["g"][:3]) / F64(F32(0.1))), rtol=0, atol=1e-7)


def test_info_step_rank_zero_and_thresholds():
    pose = _pose(9)
    zero = np.zeros(1, _lib.POSE_INFO)[0]
    zero["c"], zero["rho"], zero["g"] = F32([0, 0, 1]), F32(0.1), np.ones(6)
    got, delta, rank = api.information_step(zero, api.information_eig(zero)[0], pose[None], 1e-6)
    assert rank[0] == 0 and not delta.any() and got[0].tobytes() == pose.tobytes()      # rank 0: the identity
    # a direction below min_ratio gets delta = 0 exactly
    info = np.zeros(1, _lib.POSE_INFO)[0]
    lam = [1e-9, 1.0, 2.0, 3.0, 4.0, 5.0]
    Hm = np.diag(lam)
    info["H"], info["g"], info["c"], info["rho"] = Hm[np.triu_indices(6)], np.ones(6), F32([0, 0, 1]), F32(0.1)
    eig = api.information_eig(info)[0]
    _, delta, rank = api.information_step(info, eig, pose[None], 1e-6)
    assert rank[0] == 5 and delta[0][0] == 0.0 and np.allclose(delta[0][1:], 1.0 / np.array(lam[1:]), rtol=1e-15)
    _, delta, rank = api.information_step(info, eig, pose[None], 0.0)
    assert rank[0] == 6 and delta[0][0] == 1.0 / 1e-9
    lib = _lib.load()
    out, p = np.zeros(16, F32), np.ascontiguousarray(pose)
    i1, e1 = np.array([info]), np.array([eig])
    for args in ((None, _lib.ptr(e1), 0.0, _lib.ptr(p), _lib.ptr(out), None, None), (_lib.ptr(i1), None, 0.0, _lib.ptr(p), _lib.ptr(out), None, None),
                 (_lib.ptr(i1), _lib.ptr(e1), 0.0, None, _lib.ptr(out), None, None), (_lib.ptr(i1), _lib.ptr(e1), 0.0, _lib.ptr(p), None, None, None),
                 (_lib.ptr(i1), _lib.ptr(e1), -1e-9, _lib.ptr(p), _lib.ptr(out), None, None), (_lib.ptr(i1), _lib.ptr(e1), float("nan"), _lib.ptr(p), _lib.ptr(out), None, None)):
        assert lib.pr_info_step(*args) == _lib.PR_ERR_INVALID
    assert not out.any()
    assert lib.pr_info_step(_lib.ptr(i1), _lib.ptr(e1), 0.0, _lib.ptr(p), _lib.ptr(out), None, None) == _lib.PR_OK and out.any()


# ---- the plate on the wall, through the reference loop ---------------------------------------------------------------------------------------------
def plate_reference_run():
    P = CF.PLATE
    W, H, K = P["W"], P["H"], P["K"]
    tris, proj = CF.plate_tris(), O.compute_proj(K, W, H)
    true, start = CF.plate_poses()
    scene = CF.plate_scene(O.render(tris, true[None], W, H, proj)[0])
    N = CF.nearest_ref(scene, P["jump"], P["radius"])
    cm = np.zeros(3, F32)

    def surface(poses):
        return CF.plane_surface(O.render(tris, poses, W, H, proj), scene, K, CF.centers(poses, cm), P["rho"], P["max_dist_diff"])

    def contour(poses):
        cs = CF.centers(poses, cm)
        recs = CF.fit_records(O.render(tris, poses, W, H, proj), scene, N, P["tau"], P["jump"], K, cs, P["rho"])
        return [(r, CF.info_of(r, cs[i], P["rho"])) for i, r in enumerate(recs)]
    poses, hist = CF.refine(surface, contour, start[None], P["iterations"], P["weight"], P["min_ratio"], P["min_used"])
    return true, start, poses[0], hist


def assert_plate_conditions(true, start, final, surface_lambda, combined_rank, what):
    """The conditions of the plate case, the same for the reference loop and for api.refine_contours."""
    t0, r0 = CF.plate_errors(start, true)
    t1, r1 = CF.plate_errors(final, true)
    print(what, "in-plane translation", t0, "->", t1, "mm; in-plane rotation", r0, "->", r1, "rad; surface lambda", surface_lambda, "rank", combined_rank)
    assert abs(t0 - 30.0) < 0.5 and abs(r0 - 0.05) < 1e-3
    assert (surface_lambda[:3] <= 1e-12 * surface_lambda[5]).all() and surface_lambda[3] > 1e-6 * surface_lambda[5], what
    assert combined_rank == 6, what
    assert t1 <= t0 / 10.0, what
    assert r1 < r0 / 2.0, what


def test_plate_on_wall_through_the_reference_loop():
    true, start, final, hist = plate_reference_run()
    assert (hist["used"] >= CF.PLATE["min_used"]).all()
    assert_plate_conditions(true, start, final, hist["surface_lambda"][0, 0], int(hist["rank"][0, 0]), "reference loop")
    assert (hist["rank"] == 6).all()
    assert hist["rms_px"][-1, 0] < hist["rms_px"][0, 0] / 4.0       # the contour's RMS pixel distance falls with the pose error
