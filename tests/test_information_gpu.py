"""GPU tests (-m gpu) of pose observability (pr_pose_info / pr_pose_eig, include/pose_refine.h) against tests/info_ref.py: the float64 sums of the
information pass on the four scene forms, what the eigen kernel's outputs must satisfy, the analytic null spaces, batches, the fused and mixed
forms, and the neighbours the calls must leave alone.

Correspondences are the library's own for projective and kd-tree scenes (corr_host of a PR_ROBUST_NONE call to pr_debug_robust_terms, which
tests/test_robust_gpu.py ties to the tested pass) and numpy's for the closest-point grid (grid_ref.associate).  The reference forms every term with
the header's operations, so device and reference differ only in the order of the additions: each sum lies within info_ref.sum_bound of math.fsum."""
import numpy as np
import pytest

import grid_ref
import info_ref as I
import robust_ref as R
import seam_cases as S
import truth_cases as TC
import truth_ref as T
from gpu_common import H, W
from pass_sums_ref import window
from pose_refine_amd import _lib, api, synth
from test_pass_sums_gpu import options, ragged
from verify_ref import launch_split_case

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZES = (1, 5, 6, 7, 64, 65, 257, 1025, 3073, 6145)              # the 6-parameter edge, a wavefront, a workgroup, a 1024-point step, several blocks (2048 points each)
KINDS = (R.NONE, R.HUBER, R.TUKEY, R.CAUCHY)
RHO = 0.1


def dv(cloud):
    return api.DeviceVector.from_host(np.ascontiguousarray(cloud, F32).reshape(-1))


def lib_associate(scene, packed):
    none = api.Robust(api.ROBUST_NONE)

    def associate(cloud):
        _, corr = api.debug_robust_terms(dv(cloud), scene, none, packed=packed)
        return corr[:, 0:3].copy(), corr[:, 4:7].copy(), corr[:, 3] == 1.0
    return associate


class Kit:
    def __init__(self, scene, packed=False, grid_host=None):
        self.scene, self.packed = scene, packed
        self.associate = R.grid_associate(*grid_host) if grid_host else lib_associate(scene, packed)

    def information(self, flat, offs, centers, radii, robust=None, want_eig=True):
        return api.icp_information(dv(flat), offs, self.scene, centers, radii, robust=robust, want_eig=want_eig, packed=self.packed)


@pytest.fixture(scope="module")
def kits(gpu, gscenes):
    g = api.Scene_grid.from_scene_nn(gscenes["nn"], 0.004)
    host = (grid_ref.from_ctypes(g.desc()), g.cell_points().reshape(-1), g.records())
    return {"proj": Kit(gscenes["proj"]), "packed": Kit(gscenes["proj"], packed=True), "nn": Kit(gscenes["nn"]), "grid": Kit(g, grid_host=host)}


def centre_of(cloud):
    return np.asarray(cloud, F32).reshape(-1, 3).astype(F64).mean(0).astype(F32)


def assert_record(info, ref, what):
    """Counts exact; every sum within (n_valid + 16) * 2^-52 * sum |term| of the reference's fsum."""
    assert (int(info["n_points"]), int(info["n_valid"]), int(info["n_zero_weight"])) == (ref["n_points"], ref["n_valid"], ref["n_zero_weight"]), what
    got = I.flat_sums(info)
    err, bound = np.abs(got - ref["sums"]), I.sum_bound(ref["n_valid"], ref["abs"])
    assert (err <= bound).all(), (what, "columns", np.flatnonzero(err > bound), err[err > bound], bound[err > bound])
    return float((err / np.where(bound > 0, bound, 1.0)).max())


def assert_eig(info, eig, what):
    """What a decomposition must satisfy -- never eigh's vectors: a degenerate subspace has no unique basis."""
    Hm, lam, V = I.sym6(info["H"]), np.asarray(eig["lambda"], F64), np.asarray(eig["V"], F64).reshape(6, 6)
    top = lam[5]
    res = float(np.abs(Hm @ V - V * lam[None, :]).max())
    orth = float(np.abs(V.T @ V - np.eye(6)).max())
    dl = float(np.abs(lam - np.linalg.eigvalsh(Hm)).max())
    print(what, "residual", res, "orthogonality", orth, "lambda - eigh", dl, "lambda[5]", top, "sweeps", int(eig["sweeps"]))
    assert res <= 1e-12 * top and orth <= 1e-12 and dl <= 1e-12 * top, what
    assert (np.diff(lam) >= 0).all() and int(eig["sweeps"]) <= _lib.INFO_MAX_SWEEPS, what
    for k in range(6):                                               # the sign rule: the first component of largest magnitude is positive
        assert V[int(np.argmax(np.abs(V[:, k]))), k] > 0, (what, k)
    if int(info["n_valid"]) == 0:
        assert not lam.any() and np.array_equal(V, np.eye(6)) and int(eig["sweeps"]) == 0, what


# ---- 1. sums against the reference, 2. eigen outputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proj", "packed", "nn", "grid"])
def test_sums_follow_the_reference_and_eigenpairs_hold(kits, scenario, name):
    kit = kits[name]
    worst = 0.0
    for n in SIZES:
        cloud = np.ascontiguousarray(window(scenario["cloud"], n), F32)
        before = cloud.copy()
        corr = kit.associate(cloud)
        a = np.abs(R.residuals(cloud, corr)[corr[2]])
        assert len(a) > 0, (name, n)
        scale = float(np.median(a.astype(F64))) or 0.001             # the robust scale at the median |r| of the window: both sides of it are populated
        c = centre_of(cloud)
        for kind in KINDS:
            rb = api.Robust(kind, scale) if kind != R.NONE else None
            info, eig = kit.information(cloud, [0, n], c[None], [RHO], robust=rb)
            ref = I.record(cloud, corr, rb, c, RHO)
            what = (name, n, kind)
            worst = max(worst, assert_record(info[0], ref, what))
            assert np.array_equal(info[0]["c"], c) and info[0]["rho"] == F32(RHO) and info[0]["reserved"] == 0
            assert_eig(info[0], eig[0], what)
            if kind == R.TUKEY and n >= 64:
                assert 0 < ref["n_zero_weight"] < ref["n_valid"], what
            only, none = kit.information(cloud, [0, n], c[None], [RHO], robust=rb, want_eig=False)
            assert none is None and only.tobytes() == info.tobytes(), what
        assert np.array_equal(cloud, before)
    print(name, "largest error / bound", worst)


# ---- 3. truth: analytic scenes, every point associated, the null spaces of the host test -----------------------------------------------------
def analytic_scene(depth_mm, normals):
    """A projective scene from arrays: pcd = the pixel rays times the analytic depth (metres), normal = the analytic unit normals."""
    K = TC.NORMAL_K
    rays = T._pixel_rays(K, TC.NORMAL_W, TC.NORMAL_H)
    hit = depth_mm > 0
    pts = np.where(hit[..., None], rays * (depth_mm / 1000.0)[..., None], 0.0)
    sc = api.Scene_projective()
    sc.width, sc.height, sc.max_dist_diff, sc.K = TC.NORMAL_W, TC.NORMAL_H, 0.1, np.asarray(K, F32).reshape(-1)
    sc.pcd_buffer, sc.normal_buffer = dv(pts.reshape(-1, 3)), dv(np.where(hit[..., None], normals, 0.0).reshape(-1, 3))
    return sc, pts[hit], normals[hit]


@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_truth_null_spaces(gpu, name):
    K = TC.NORMAL_K
    if name == "plane":
        z, nt = T.plane_depth(K, TC.NORMAL_W, TC.NORMAL_H, (0, 0, -1), 800.0)
        c, rho, null = (0.0, 0.0, 0.8), 0.1, [2, 3, 4]
    else:
        z, nt = T.sphere_depth(K, TC.NORMAL_W, TC.NORMAL_H, (6.0, -4.0, 900.0), 150.0)
        c, rho, null = (0.006, -0.004, 0.9), 0.15, [0, 1, 2]
    scene, pts, nrm = analytic_scene(z, nt)
    cloud = (pts + 0.001 * nrm).astype(F32)                          # the scene's own points moved 1 mm along their normals
    n = len(cloud)
    assert n > 2000
    _, corr = api.debug_robust_terms(dv(cloud), scene, api.Robust(api.ROBUST_NONE))
    assert (corr[:, 3] == 1.0).all() and np.array_equal(corr[:, 0:3], pts.astype(F32)), name      # every point associates, with the point it came from
    for packed in (False, True):
        info, eig = api.icp_information(dv(cloud), [0, n], scene, [c], [rho], packed=packed)
        assert int(info[0]["n_valid"]) == n == int(info[0]["n_points"]), (name, packed)
        assert_eig(info[0], eig[0], (name, packed))
        lam = np.asarray(eig[0]["lambda"])
        bound = I.null_bound(float(np.abs(cloud).max()), rho, float(info[0]["sum_w"]))
        print(name, packed, "lambda / lambda[5]", lam / lam[5], "bound / lambda[5]", bound / lam[5])
        assert (np.abs(lam[:3]) <= bound).all() and lam[3] > 1e6 * bound, (name, packed, lam, bound)
        want = I._span_projector(np.eye(6)[null])
        assert np.abs(I.projector(eig[0]["V"], range(3)) - want).max() <= 1e-6, (name, packed)
        assert list(api.observable_rank(eig, 1e-9)) == [3] and len(api.filter_by_observability([0], eig, 1e-9)) == 0


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proj", "grid", "nn"])
@pytest.mark.parametrize("n_clouds", [1, 3, 65])
def test_batches_equal_the_single_calls(kits, scenario, name, n_clouds):
    """Ragged clouds, an empty one and one without a single valid correspondence among them: every record is the one-cloud call's, byte for byte,
    and a second call returns the same bytes."""
    kit = kits[name]
    src = np.ascontiguousarray(scenario["cloud"], F32)
    sizes = [(2049, 0, 7, 1025, 3073, 1, 65, 257, 4097, 6)[i % 10] + (i // 10) for i in range(n_clouds)]
    parts = [src[12001 + (131 * i) % 9000:12001 + (131 * i) % 9000 + s] for i, s in enumerate(sizes)]      # (from the part of the cloud that projects onto the scene)
    if n_clouds >= 3:
        parts[2] = parts[2] + F32(10.0)                              # ten metres off: nothing associates
    flat, offs = ragged(parts)
    centers = np.array([centre_of(p) if len(p) else (0, 0, 0.8) for p in parts], F32)
    radii = np.array([0.05 + 0.01 * (i % 5) for i in range(n_clouds)], F32)
    rb = api.Robust(api.ROBUST_HUBER, 0.004)
    info, eig = kit.information(flat, offs, centers, radii, robust=rb)
    again, eagain = kit.information(flat, offs, centers, radii, robust=rb)
    assert info.tobytes() == again.tobytes() and eig.tobytes() == eagain.tobytes()
    assert np.array_equal(info["n_points"], sizes)
    for i, p in enumerate(parts):
        one, eone = kit.information(p.reshape(-1, 3), [0, len(p)], centers[i:i + 1], radii[i:i + 1], robust=rb)
        assert one[0].tobytes() == info[i].tobytes() and eone[0].tobytes() == eig[i].tobytes(), (name, n_clouds, i, len(p))
    if n_clouds >= 3:
        for i in (1, 2):                                             # the empty cloud, the cloud nothing associates with
            z = info[i].copy()
            assert int(z["n_valid"]) == 0 and not I.flat_sums(z).any() and np.array_equal(z["c"], centers[i]) and z["rho"] == radii[i], i
            assert not np.asarray(eig[i]["lambda"]).any() and np.array_equal(eig[i]["V"], np.eye(6)) and int(eig[i]["sweeps"]) == 0, i
        assert int(info[0]["n_valid"]) > 6


def test_kdtree_routes_return_the_same_bytes(kits, scenario):
    """A kd-tree scene with compact records goes through the search kernels and the pass over their winners; without them (nn_compact 0) every lane
    walks the tree itself.  The same winners in the same order of addition: the same bytes."""
    parts = [np.ascontiguousarray(window(scenario["cloud"], n), F32) for n in (3073, 65, 1, 2049)]
    flat, offs = ragged(parts)
    centers, radii = np.array([centre_of(p) for p in parts], F32), np.full(len(parts), RHO, F32)
    rb = api.Robust(api.ROBUST_CAUCHY, 0.004)
    info, eig = kits["nn"].information(flat, offs, centers, radii, robust=rb)
    with options(nn_compact=0):
        walk, ewalk = kits["nn"].information(flat, offs, centers, radii, robust=rb)
    again, _ = kits["nn"].information(flat, offs, centers, radii, robust=rb)
    assert (info["n_valid"] > 0).all() and info.tobytes() == walk.tobytes() == again.tobytes() and eig.tobytes() == ewalk.tobytes()


# ---- 5. fused and mixed ------------------------------------------------------------------------------------------------------------------------
def camera_centres(poses, center_model):
    p = np.asarray(poses, F32).reshape(-1, 4, 4).astype(F64)
    cm = np.asarray(center_model, F32).astype(F64)
    v = ((p[:, :3, 0] * cm[0] + p[:, :3, 1] * cm[1]) + p[:, :3, 2] * cm[2]) + p[:, :3, 3]
    return (v / 1000.0).astype(F32)


@pytest.mark.parametrize("roi", [None, (160, 80, 320, 240)], ids=["full-frame", "roi"])
def test_fused_call_equals_the_cloud_call_on_its_clouds(gpu, model, scenario, gscenes, roi):
    poses = synth.hypotheses(8)
    K, proj = scenario["K"], scenario["proj"]
    rb = api.Robust(api.ROBUST_TUKEY, 0.01)
    info, eig, sizes = api.pose_information(model, poses, W, H, proj, K, gscenes["proj"], roi=roi, robust=rb)
    _, rsizes = api.refine_batch(model, poses, W, H, proj, K, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 0), roi=roi)
    assert np.array_equal(sizes, rsizes) and np.array_equal(info["n_points"], sizes) and sizes.min() > 3072
    cm = 0.5 * (np.asarray(model.bbox_min, F64) + np.asarray(model.bbox_max, F64))
    rad = F32(0.5 * float(np.linalg.norm(np.asarray(model.bbox_max, F64) - np.asarray(model.bbox_min, F64))) / 1000.0)
    centers = camera_centres(poses, cm)
    assert np.array_equal(info["c"], centers) and (info["rho"] == rad).all()
    oroi = roi or (0, 0, 0, 0)
    rw, rh = (oroi[2], oroi[3]) if roi else (W, H)
    depth = api.render(model, poses, W, H, proj, oroi)
    kit = Kit(gscenes["proj"], packed=True)
    for i in range(len(poses)):
        cl = api.depth2cloud(depth, rw, rh, K, 1, oroi[0], oroi[1], offset_elems=i * rw * rh)
        cloud = cl.to_host().reshape(-1, 3)
        assert len(cloud) == sizes[i]
        one, eone = api.icp_information(cl, [0, len(cloud)], gscenes["proj"], centers[i:i + 1], [rad], robust=rb, packed=True)
        ref = I.record(cloud, kit.associate(cloud), rb, centers[i], rad)
        assert_record(one[0], ref, ("cloud call", i))
        assert_record(info[i], ref, ("fused call", i))               # the same points in another order: the same counts, sums within the same bound
        assert_eig(info[i], eig[i], ("fused", i))
    plain, _, _ = api.pose_information(model, poses, W, H, proj, K, gscenes["proj"], roi=roi, want_eig=False)
    assert (plain["sum_w"] == plain["n_valid"]).all() and (plain["n_zero_weight"] == 0).all() and (info["n_valid"] == plain["n_valid"]).all()


def test_mixed_batch_equals_the_single_mesh_calls(gpu, model, scenario, gscenes):
    small = api.Model(tris=np.ascontiguousarray(model.tris * F32(0.9)))
    meshes = [model, small]
    idx = np.array([0, 1, 1, 0, 1, 0], np.uint32)
    poses = synth.hypotheses(6)
    args = (W, H, scenario["proj"], scenario["K"], gscenes["proj"])
    info, eig, sizes = api.pose_information_multi(meshes, idx, poses, *args)
    for m in (0, 1):
        sel = np.flatnonzero(idx == m)
        i1, e1, s1 = api.pose_information(meshes[m], poses[sel], *args)
        assert info[sel].tobytes() == i1.tobytes() and eig[sel].tobytes() == e1.tobytes() and np.array_equal(sizes[sel], s1), m
    assert info[1]["rho"] != info[0]["rho"]                          # each mesh brought its own radius


# ---- 6. untouched neighbours ----------------------------------------------------------------------------------------------------------------------
def test_calls_leave_their_neighbours_alone(gpu, model, scenario, gscenes):
    cloud = np.ascontiguousarray(window(scenario["cloud"], 3073), F32)
    d = dv(cloud)
    api.icp_information(d, [0, 3073], gscenes["proj"], [centre_of(cloud)], [RHO], robust=api.Robust(api.ROBUST_CAUCHY, 0.005))
    assert d.to_host().tobytes() == cloud.tobytes()                  # the cloud buffer, bit for bit
    poses = synth.hypotheses(4)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 4)
    args = (model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"])
    before, bsizes = api.refine_batch(*args, crit)
    api.pose_information(*args)
    api.icp_information(d, [0, 3073], gscenes["nn"], [centre_of(cloud)], [RHO])
    after, asizes = api.refine_batch(*args, crit)
    assert before.tobytes() == after.tobytes() and np.array_equal(bsizes, asizes)


# ---- 7. the 32768-cloud launch seam ---------------------------------------------------------------------------------------------------------------
def _info_rows(info, eig):
    return np.concatenate([S.byte_rows(info), S.byte_rows(eig)], axis=1)


def _seam_kit(name):
    sc = S.device_scenes()
    if name == "grid":
        return Kit(sc["grid"], grid_host=sc["grid_host"])
    return Kit(sc["proj" if name in ("proj", "packed") else "nn"], packed=name == "packed")


@pytest.mark.parametrize("name", ["proj", "packed", "nn", "nn-walk", "grid"])
def test_batch_of_two_launches(gpu, name):
    """32768 + 5 clouds in one call: the information pass runs in two pieces, each with its own staged records and its own part of the output.
    The clouds are the eight emitted clouds of verify_ref.launch_split_case through seam_cases.seam_index -- behind the seam every cloud, centre
    and radius is the next one -- so cloud 32768 + j never expects cloud j's record.  The eight-cloud call is held to info_ref; every record and
    eigen-decomposition of the large call is that of its cloud in the eight-cloud call, byte for byte."""
    kit = _seam_kit(name.split("-")[0])
    clouds = S.split_clouds()
    centers8 = np.array([centre_of(x) for x in clouds], F32)
    radii8 = np.array([0.05 + 0.01 * k for k in range(8)], F32)
    rb = api.Robust(api.ROBUST_HUBER, 0.004)
    with options(**({"nn_compact": 0} if name == "nn-walk" else {})):  # without compact records every lane walks the tree itself
        flat8, offs8 = ragged(clouds)
        info8, eig8 = kit.information(flat8, offs8, centers8, radii8, robust=rb)
        for k, cl in enumerate(clouds):
            assert_record(info8[k], I.record(cl, kit.associate(cl), rb, centers8[k], radii8[k]), (name, k))
            assert_eig(info8[k], eig8[k], (name, k))
        assert (info8["n_valid"] > 0).sum() >= 6
        idx = S.seam_index(S.P, 8)
        rows8 = _info_rows(info8, eig8)
        S.assert_seam_visible(rows8, idx)
        flat, offs = ragged([clouds[k] for k in idx])
        info, eig = kit.information(flat, offs, centers8[idx], radii8[idx], robust=rb)
    S.seam_report(("information", name), [len(x) for x in clouds], np.stack([info["n_points"], info["n_valid"]], 1), idx)
    S.assert_records_take(_info_rows(info, eig), rows8, idx)


def test_fused_and_mixed_batches_of_two_launches(gpu):
    """pose_information and pose_information_multi at 32768 + 5 hypotheses (the box and a copy scaled by 0.8, in runs of five): the eight-hypothesis
    calls are held to info_ref on the oracle's clouds; every record of the large calls is that of its mesh and pose, byte for byte."""
    import oracle_lib as O
    c, sc = launch_split_case(), S.device_scenes()
    meshes = [c["tris"], S.small_mesh(c["tris"])]
    cms, rads = np.array([[0, 0, 0], [3, -2, 1]], F32), np.array([0.08, 0.064], F32)
    kit = Kit(sc["proj"], packed=True)
    args = (c["W"], c["H"], c["proj"], S.SPLIT_K, sc["proj"])
    per_mesh = []
    for m in (0, 1):
        info8, eig8, sizes8 = api.pose_information(meshes[m], c["poses"], *args, center=cms[m], radius=float(rads[m]))
        centers = camera_centres(c["poses"], cms[m])
        assert np.array_equal(info8["c"], centers) and (info8["rho"] == rads[m]).all()
        for k, depth in enumerate(O.render(meshes[m], c["poses"], c["W"], c["H"], c["proj"])):
            cl = O.depth2cloud(depth, S.SPLIT_K)
            assert sizes8[k] == len(cl)
            assert_record(info8[k], I.record(cl, kit.associate(cl), None, centers[k], rads[m]), ("fused", m, k))
            assert_eig(info8[k], eig8[k], ("fused", m, k))
        per_mesh.append(np.concatenate([_info_rows(info8, eig8), S.byte_rows(sizes8)], axis=1))
    idx, mi = S.seam_index(S.P, 8), S.mesh_runs(S.P)
    S.assert_seam_visible(per_mesh[0], idx)
    info, eig, sizes = api.pose_information(meshes[0], c["poses"][idx], *args, center=cms[0], radius=float(rads[0]))
    S.seam_report("pose_information", per_mesh[0][:, -4:].copy().view(np.uint32).reshape(-1), np.stack([sizes, info["n_valid"]], 1), idx)
    S.assert_records_take(np.concatenate([_info_rows(info, eig), S.byte_rows(sizes)], axis=1), per_mesh[0], idx)
    table, take = S.mixed_table(per_mesh, mi, idx)
    S.assert_seam_visible(table, take)
    info, eig, sizes = api.pose_information_multi(meshes, mi, c["poses"][idx], *args, centers=cms, radii=rads)
    S.seam_report("pose_information_multi", [t[:, -4:].copy().view(np.uint32).reshape(-1).tolist() for t in per_mesh], np.stack([sizes, info["n_valid"]], 1), take)
    S.assert_records_take(np.concatenate([_info_rows(info, eig), S.byte_rows(sizes)], axis=1), table, take)
