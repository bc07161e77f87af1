"""GPU tests (-m gpu) of the closest-point grid scene (pr_scene_grid) against tests/grid_ref.py: the build cell by cell (no cell skipped), the
per-point terms, the 29 sums of every pass, the refinement loop through every entry point, and a scene on which the grid IS the exact search.
Scenes hold at most 2 000 points and grids at most 32 x 32 x 32 cells; every comparison of device output is bit for bit except the transforms of
the loop (1e-4, the suite's parity rule)."""
import numpy as np
import pytest

import grid_ref
import nn_ref
import oracle_lib as O
from gpu_common import TOL_T, brute_force_first_minimum, inliers, make_scene, random_mesh
from pass_sums_ref import differing_columns, u32
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = grid_ref.NONE
CELL64 = F32(1.0 / 64)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def build(pts, nrm, lo, hi, cell, mdd, reach=None, max_leaf=10):
    """(kd-tree scene, grid scene, the grid's geometry as grid_ref sees it, points and normals in tree order)."""
    pts, nrm = np.ascontiguousarray(pts, F32).copy(), np.ascontiguousarray(nrm, F32).copy()
    scene = make_scene(pts, nrm, max_leaf, mdd)                    # (reorders pts / nrm in place: tree order)
    grid = api.Scene_grid.from_scene_nn(scene, float(cell), reach=reach, lo=lo, hi=hi)
    desc = grid_ref.from_ctypes(grid.desc())
    assert max(desc.dim) <= 32 and len(pts) <= 2000
    return scene, grid, desc, pts, nrm


def auto_box(pts, mdd):
    """AABB grown by mdd and the cell that gives it at most 32 cells a side."""
    lo, hi = pts.min(0).astype(np.float64) - mdd, pts.max(0).astype(np.float64) + mdd
    return lo, hi, float((hi - lo).max()) / 31.0


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def clutter_points():
    """A wavy surface with a raised box (depth edges), noise and holes, seen by a 48 x 40 camera: nn_ref's clutter at this file's size."""
    W, H = 48, 40
    K = nn_ref.kvec(50.0, 50.0, 24.0, 20.0)
    depth = nn_ref.compose(nn_ref.box_layer(W, H, (10, 24, 8, 26), 380.0, slope=0.8), nn_ref.wavy(W, H, 520.0, 60.0, tilt=(0.6, 0.3)))
    depth = nn_ref.perturb(depth, np.random.default_rng(3))
    pts = O.depth2cloud(depth, K)
    return pts, _unit(np.random.default_rng(4).normal(size=(len(pts), 3)))


def planted_points():
    """Dyadic coordinates in a 16^3 grid of cell 1/64 at the origin: A alone at the centre of cell (4, 4, 4) -- centres three cells away along an
    axis are at EXACTLY 3/64 --, a pair mirrored in x about the centre of (11, 11, 11) and one mirrored in y about the centre of (11, 4, 11): every
    centre on their mirror planes is at bitwise equal distance from both."""
    c = lambda i, j, k: np.array([i + 0.5, j + 0.5, k + 0.5]) / 64.0
    pts = np.array([c(4, 4, 4), c(11, 11, 11) + [1 / 256, 0, 0], c(11, 11, 11) - [1 / 256, 0, 0],
                    c(11, 4, 11) + [0, 1 / 128, 0], c(11, 4, 11) - [0, 1 / 128, 0]], F32)
    return pts, _unit(np.random.default_rng(5).normal(size=(len(pts), 3)))


def mixed_points():
    """For the per-point and pass tests, in a 32 x 16 x 16 grid of cell 1/64 at (-0.25, -0.125, 0.375): a smooth surface with a step over
    x < 0.05 (analytic normals) and two isolated points at the centres of cells (26, 8, 8) and (28, 8, 2), whose y is 1/128: a query 1/32 =
    max_dist_diff below them in y is answered by them, at a distance a few ulps either side of the radius."""
    rng = np.random.default_rng(6)
    n = 1400
    x, y = rng.uniform(-0.2, 0.05, n), rng.uniform(-0.1, 0.1, n)
    z = 0.5 + 0.02 * np.sin(12 * x) * np.cos(9 * y) - 0.06 * ((x > -0.1) & (x < -0.05))
    nrm = _unit(np.stack([-0.24 * np.cos(12 * x) * np.cos(9 * y), 0.18 * np.sin(12 * x) * np.sin(9 * y), np.ones(n)], 1))
    iso = (np.array([[26.5, 8.5, 8.5], [28.5, 8.5, 2.5]]) / 64.0 + [-0.25, -0.125, 0.375])
    pts = np.concatenate([np.stack([x, y, z], 1), iso]).astype(F32)
    nrm = np.concatenate([nrm, _unit(np.array([[0.1, 0.9, 0.2], [0.0, -1.0, 0.3]]))]).astype(F32)
    return pts, nrm, iso.astype(F32)


MIXED_LO, MIXED_HI, MIXED_MDD = (-0.25, -0.125, 0.375), (-0.25 + 31.5 / 64, -0.125 + 15.5 / 64, 0.375 + 15.5 / 64), 1.0 / 32


@pytest.fixture(scope="module")
def mixed(gpu):
    pts, nrm, iso = mixed_points()
    scene, grid, desc, pts, nrm = build(pts, nrm, MIXED_LO, MIXED_HI, CELL64, MIXED_MDD)
    assert desc.dim == (32, 16, 16)
    cp, rec = grid.cell_points().reshape(-1), grid.records()
    cp.setflags(write=False); rec.setflags(write=False)
    return dict(scene=scene, grid=grid, desc=desc, pts=pts, nrm=nrm, iso=iso, cp=cp, rec=rec)


# ---- 1. the build ---------------------------------------------------------------------------------------------------------------------
def check_build(pts, nrm, lo, hi, cell, mdd, reach=None):
    scene, grid, desc, pts, nrm = build(pts, nrm, lo, hi, cell, mdd, reach)
    cp = grid.cell_points()
    assert cp.shape == desc.dim[::-1] and cp.size == np.prod(desc.dim)
    bf = grid_ref.expected_cells(desc, pts)
    bad = grid_ref.check_cells(cp, bf)                               # every cell: none is skipped
    assert not bad, (len(bad), [(c, int(cp.reshape(-1)[c]), bf.ties[c][:4], bool(bf.inside[c]), float(bf.d2[c])) for c in bad[:6]])
    rec = grid.records()
    assert rec.shape == (len(pts), 8) and grid.desc().n_points == len(pts)
    assert np.array_equal(u32(rec[:, 0:3]), u32(pts)) and np.array_equal(u32(rec[:, 4:7]), u32(nrm))
    assert not u32(rec[:, 3]).any() and not u32(rec[:, 7]).any()
    assert grid.nbytes == cp.size * 4 + len(pts) * 32
    again = api.Scene_grid.from_scene_nn(scene, float(cell), reach=reach, lo=lo, hi=hi)
    assert again.cell_points().tobytes() == cp.tobytes() and again.records().tobytes() == rec.tobytes()
    return desc, cp.reshape(-1), bf, pts


def test_build_clutter(gpu):
    pts, nrm = clutter_points()
    assert 1500 < len(pts) <= 2000
    lo, hi, cell = auto_box(pts, 0.02)
    desc, cp, bf, _ = check_build(pts, nrm, lo, hi, cell, 0.02)
    assert (cp == NONE).sum() > 1000 and (cp != NONE).sum() > 1000 and np.prod(desc.dim) > 8000


@pytest.mark.parametrize("kind", ["coplanar", "collinear", "repeated"])
def test_build_degenerate(gpu, kind):
    fam = nn_ref.degenerate(kind)
    pts, nrm = fam.pts[:2000], fam.nrm[:2000]
    lo, hi, cell = auto_box(pts, 0.01)
    desc, cp, bf, _ = check_build(pts, nrm, lo, hi, cell, 0.01)
    assert (cp != NONE).any()
    if kind == "repeated":                                         # 500 copies of one point: every non-empty cell's tie set is all of them
        assert (bf.n_ties()[bf.inside] == 500).all()


@pytest.mark.parametrize("side", [-1, 0, 1])
def test_build_planted_ties_and_reach(gpu, side):
    """Exact float32 ties on the mirror planes, and reach = 3/64 moved by `side` ulps: the centres exactly 3/64 from A are inside reach only for +1
    (d2 == reach * reach fails the '<')."""
    pts, nrm = planted_points()
    reach = F32(3.0 / 64)
    reach = reach if side == 0 else np.nextafter(reach, F32(1.0) if side > 0 else F32(0.0))
    desc, cp, bf, tpts = check_build(pts, nrm, (0, 0, 0), (15.5 / 64, 15.5 / 64, 15.5 / 64), CELL64, 1.0 / 64, reach=float(reach))
    assert desc.dim == (16, 16, 16) and F32(desc.reach) == reach
    assert ((bf.n_ties() > 1) & bf.inside).sum() >= 20                 # the premise: exact ties exist inside reach
    a = int(np.flatnonzero((tpts == np.array([4.5, 4.5, 4.5], F32) / 64).all(1))[0])
    cell = lambda i, j, k: i + 16 * (j + 16 * k)
    three_away = [cell(7, 4, 4), cell(1, 4, 4), cell(4, 7, 4), cell(4, 1, 4), cell(4, 4, 7), cell(4, 4, 1)]
    assert (bf.d2[three_away] == F32(9.0 / 4096)).all()
    assert (cp[three_away] == (a if side > 0 else NONE)).all()
    assert cp[cell(4, 4, 4)] == a and cp[cell(6, 4, 4)] == a and cp[cell(15, 15, 0)] == NONE


# ---- 2. per-point terms ---------------------------------------------------------------------------------------------------------------
def hard_cloud(m):
    """3 000 points: near the surface, outside each face, on cell boundaries and far faces, in NONE cells, a few ulps either side of the
    acceptance radius, NaN / +-inf / denormal coordinates."""
    desc, rng = m["desc"], np.random.default_rng(9)
    o, c = desc.origin.astype(np.float64), float(desc.cell)
    ext = np.array(desc.dim) * c
    parts = []
    near = m["pts"][rng.integers(0, len(m["pts"]), 2200)].astype(np.float64) + rng.normal(size=(2200, 3)) * 0.012
    parts.append(near)
    inside_pt = o + ext * [0.3, 0.5, 0.55]
    for a in range(3):                                             # outside each of the six faces
        for s, v in ((0, o[a] - 0.001), (1, o[a] + ext[a] + 0.001), (0, o[a] - 5.0), (1, o[a] + ext[a] + 5.0)):
            p = np.tile(inside_pt, (10, 1)) + rng.normal(size=(10, 3)) * 0.01
            p[:, a] = v
            parts.append(p)
    edge = []
    for a in range(3):                                             # exactly on cell boundaries and on both faces: f == 0 is inside, f == dim is not
        for i in (0, 1, 7, desc.dim[a] - 1, desc.dim[a]):
            p = inside_pt.copy(); p[a] = float(F32(desc.origin[a]) + F32(i) * desc.cell)
            edge.append(p)
            q = p.copy(); q[a] = float(np.nextafter(F32(p[a]), F32(-10.0)))
            edge.append(q)
    parts.append(np.array(edge))
    none_cells = np.flatnonzero(m["cp"] == NONE)
    assert len(none_cells) > 200
    parts.append(grid_ref.centres(desc)[none_cells[rng.integers(0, len(none_cells), 200)]].astype(np.float64))
    thr = []
    for d in m["iso"]:                                             # the winner 1/32 away in y, stepped ulp by ulp across the radius
        y = F32(d[1]) - F32(MIXED_MDD)
        for k in range(-6, 7):
            yy = y
            for _ in range(abs(k)):
                yy = np.nextafter(yy, F32(1.0) if k > 0 else F32(-1.0))
            thr.append([d[0], yy, d[2]])
    parts.append(np.array(thr, np.float64))
    cloud = np.concatenate(parts).astype(F32)
    odd = np.array([[np.nan, 0.0, 0.5], [0.0, np.nan, 0.5], [0.0, 0.0, np.nan], [np.inf, 0.0, 0.5], [-np.inf, 0.0, 0.5], [0.0, np.inf, 0.5],
                    [0.0, 0.0, -np.inf], [np.inf, -np.inf, np.nan], [1e-40, 0.0, 0.5], [-0.1, -1e-42, 0.5], [0.0, 0.0, 1e-39]], F32)
    fill = m["pts"][rng.integers(0, len(m["pts"]), 3000 - len(cloud) - len(odd))] + F32(0.002)
    cloud = np.ascontiguousarray(np.concatenate([cloud, odd, fill]).astype(F32))
    assert len(cloud) == 3000
    return cloud, len(thr)


@pytest.mark.parametrize("with_update", [False, True])
def test_per_point_terms(gpu, mixed, with_update):
    m = mixed
    cloud, n_thr = hard_cloud(m)
    upd = None
    if with_update:                                                # a pending update: 0.2 degrees about z and y, a millimetre
        a, b = np.deg2rad(0.2), np.deg2rad(-0.15)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        upd = np.eye(4, dtype=F32); upd[:3, :3] = (Rz @ Ry).astype(F32); upd[:3, 3] = [0.001, -0.0007, 0.0004]
    dev = api.DeviceVector.from_host(cloud.reshape(-1))
    got = api.debug_contrib29(dev, m["grid"], update=upd)
    moved = grid_ref.transform(cloud, upd) if with_update else cloud
    back = dev.to_host().reshape(-1, 3)
    finite = np.isfinite(moved).all(1)
    assert np.array_equal(u32(back[finite]), u32(moved[finite])) and not np.isfinite(back[~finite]).all(1).any()
    winner, valid = grid_ref.associate(moved, m["desc"], m["cp"], m["rec"])
    want = grid_ref.terms29(moved, winner, valid, m["rec"])
    assert np.array_equal(u32(got), u32(want)), np.flatnonzero((u32(got) != u32(want)).any(1))[:10]
    inside, _ = grid_ref.cell_of(moved, m["desc"])
    # the ingredients are there: outside, NONE cells, winners beyond the radius, valid ones
    assert (~inside).sum() >= 100 and (inside & (winner == NONE)).sum() >= 150 and ((winner != NONE) & ~valid).sum() >= 50 and valid.sum() >= 1000
    if not with_update:
        with np.errstate(invalid="ignore", over="ignore"):
            e = m["rec"][np.where(winner != NONE, winner, 0), 0:3] - cloud
            e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        acc = F32(MIXED_MDD) * F32(MIXED_MDD)
        close = (winner != NONE) & (np.abs(e2 - acc) <= 16 * np.spacing(acc))
        assert close.sum() >= n_thr - 2 and valid[close].any() and (~valid[close]).any() and (e2[close] == acc).any()
        on_far_face = inside_face_points(m["desc"])
        assert not grid_ref.cell_of(on_far_face, m["desc"])[0].any()


def inside_face_points(desc):
    """One point exactly on each far face (f == dim)."""
    p = np.tile((desc.origin + F32(0.1)).astype(F32), (3, 1))
    for a in range(3):
        p[a, a] = desc.origin[a] + F32(desc.dim[a]) * desc.cell
    return p


# ---- 3. pass sums ---------------------------------------------------------------------------------------------------------------------
def test_pass_sums_every_pass(gpu, mixed):
    """trace_sums (host solve) over clouds around the block boundaries, an empty cloud and one without a valid point: three passes, all 29 sums of
    every pass and hypothesis bit-equal to the canonical tree over grid_ref's terms."""
    m = mixed
    ppb = api.get_option("points_per_block")
    sizes = [1, 255, 256, 257, 1023, 1024, 1025, ppb - 1, ppb, ppb + 1, 2 * ppb + 1]
    rng = np.random.default_rng(12)
    clouds = [(m["pts"][rng.integers(0, len(m["pts"]), n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.02).astype(F32) for n in sizes]
    clouds.insert(4, np.zeros((0, 3), F32))
    clouds.append((np.tile(m["desc"].origin, (100, 1)) + F32(0.004)).astype(F32))       # inside the grid, in NONE cells
    assert not grid_ref.associate(clouds[-1], m["desc"], m["cp"], m["rec"])[1].any()
    crit = (0.0, 0.0, 2)
    flat = np.ascontiguousarray(np.concatenate(clouds), F32)
    offs = np.cumsum([0] + [len(c) for c in clouds]).astype(np.uint32)
    rows = api.trace_sums(len(clouds), 3)
    try:
        res = api.ICP_Point2Plane_batch(api.DeviceVector.from_host(flat.reshape(-1)), offs, m["grid"], api.ICPConvergenceCriteria(*crit))
    finally:
        api.trace_sums_off()
    bad = []
    for i, cl in enumerate(clouds):
        T, rmse, fit, passes, want = grid_ref.icp_loop(cl, m["desc"], m["cp"], m["rec"], crit, ppb, trace=True)
        assert passes == (0 if len(cl) == 0 else 1 if i == len(clouds) - 1 else passes) and (passes == 3 or len(cl) < 255), (i, passes)
        if len(cl) >= 255:                                         # the clouds keep valid and invalid points in every pass
            assert (want[:, 28] > 0.3 * len(cl)).all() and (want[:, 28] < 0.97 * len(cl)).all(), (i, want[:, 28])
        assert np.isnan(rows[passes:, i]).all(), (i, "a row the loop must not write")
        for it in range(passes):
            d = differing_columns(rows[it, i], want[it])
            if d:
                bad.append((it, i, len(cl), d))
        assert res[i]["fitness"] == F32(fit) and res[i]["inlier_rmse"] == F32(rmse), (i, len(cl))
        if len(cl) >= 255:
            assert np.allclose(res[i]["T"], T, rtol=0, atol=TOL_T), (i, len(cl))
    assert not bad, f"(pass, cloud, points, differing columns) = {bad[:12]}"
    assert (rows[0, :, 28][~np.isnan(rows[0, :, 28])] > 0).sum() >= len(sizes)


# ---- 4. the loop --------------------------------------------------------------------------------------------------------------------
W4, H4 = 160, 120
K4 = (synth.K_TEST.reshape(3, 3) * np.array([[0.25], [0.25], [1.0]], F32)).astype(F32).reshape(-1)
CRIT4 = (0.0, 0.0, 10)


@pytest.fixture(scope="module")
def loop(gpu):
    rng = np.random.default_rng(21)
    tris = random_mesh(rng, 400, 30.0)
    proj = O.compute_proj(K4, W4, H4)
    depth = O.render(tris, synth.scene_pose()[None], W4, H4, proj)[0]
    nrm_img = O.get_normal(depth.astype(np.uint16), K4).reshape(H4, W4, 3)
    ys, xs = np.nonzero(depth)
    pts = O.depth2cloud(depth, K4)
    assert len(pts) == len(ys) > 800
    keep = np.sort(rng.choice(len(pts), min(2000, len(pts)), replace=False))
    pts, nrm = pts[keep], np.ascontiguousarray(nrm_img[ys[keep], xs[keep]], F32)
    mdd = 0.02
    lo, hi, cell = auto_box(pts, mdd)
    scene, grid, desc, pts, nrm = build(pts, nrm, lo, hi, cell, mdd)
    poses = synth.hypotheses(8)
    clouds = [O.depth2cloud(d, K4) for d in O.render(tris, poses, W4, H4, proj)]
    return dict(tris=tris, proj=proj, poses=poses, clouds=clouds, grid=grid, desc=desc, cp=grid.cell_points().reshape(-1), rec=grid.records())


def test_loop_against_reference(gpu, loop):
    L = loop
    crit = api.ICPConvergenceCriteria(*CRIT4)
    ppb = api.get_option("points_per_block")
    res, sizes = api.refine_batch(L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
    assert np.array_equal(sizes, [len(c) for c in L["clouds"]]) and (sizes > 500).all()
    for i, cl in enumerate(L["clouds"]):
        T, rmse, fit, _ = grid_ref.icp_loop(cl, L["desc"], L["cp"], L["rec"], CRIT4, ppb)
        assert inliers(res[i]["fitness"], len(cl)) == inliers(fit, len(cl)), i
        assert np.allclose(res[i]["T"], T, rtol=0, atol=TOL_T), (i, np.abs(res[i]["T"] - T).max())
    assert (inliers(res["fitness"], sizes) > 100).sum() >= 4          # the hypotheses do meet the scene
    try:
        api.set_option("solve", api.SOLVE_DEVICE)
        dres, dsizes = api.refine_batch(L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
        api.refine_submit(0, L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
        sres_d, _ = api.refine_wait(0)
    finally:
        api.set_option("solve", api.SOLVE_HOST)
    assert dres.tobytes() == res.tobytes() and np.array_equal(dsizes, sizes)           # host and device solve agree bitwise
    assert sres_d.tobytes() == res.tobytes()


def test_loop_entry_points_agree(gpu, loop):
    L = loop
    crit = api.ICPConvergenceCriteria(*CRIT4)
    res, sizes = api.refine_batch(L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
    api.refine_submit(1, L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
    sres, ssizes = api.refine_wait(1)
    assert sres.tobytes() == res.tobytes() and np.array_equal(ssizes, sizes)
    pres, psizes = api.refine_pyramid(L["tris"], L["poses"], W4, H4, L["proj"], K4, L["grid"], levels=[(1, CRIT4)])
    assert pres.tobytes() == res.tobytes() and np.array_equal(psizes, sizes)
    other = random_mesh(np.random.default_rng(22), 300, 25.0)
    idx = np.array([0, 1, 0, 1, 1, 0, 0, 1])
    mres, msizes = api.refine_batch_multi([L["tris"], other], idx, L["poses"], W4, H4, L["proj"], K4, L["grid"], crit)
    ores, osizes = api.refine_batch(other, L["poses"][idx == 1], W4, H4, L["proj"], K4, L["grid"], crit)
    assert mres[idx == 0].tobytes() == res[idx == 0].tobytes() and np.array_equal(msizes[idx == 0], sizes[idx == 0])
    assert mres[idx == 1].tobytes() == ores.tobytes() and np.array_equal(msizes[idx == 1], osizes)
    # the single-cloud and batch entry points on one of the clouds
    cl = L["clouds"][0]
    one = api.ICP_Point2Plane(api.DeviceVector.from_host(cl.reshape(-1)), L["grid"], crit)
    assert np.array_equal(one.transformation_.reshape(-1), res[0]["T"]) and one.fitness_ == res[0]["fitness"] and one.inlier_rmse_ == res[0]["inlier_rmse"]


def test_invalid_grids_are_refused(gpu, mixed):
    lib = _lib.load()
    cloud = api.DeviceVector.from_host(np.zeros(30, F32))
    out = np.zeros(1, _lib.RESULT)
    import ctypes as C
    for field, value in (("cell_point", None), ("rec", None), ("inv_cell", 63.0), ("cell", float("nan")), ("max_dist_diff", 0.0), ("reach", float("inf")),
                         ("n_points", 0)):
        d = _lib.SceneGridDesc.from_buffer_copy(mixed["grid"].desc())
        setattr(d, field, value)
        rc = lib.pr_icp_grid(cloud.data(), 10, C.addressof(d), api.ICPConvergenceCriteria(0.0, 0.0, 1).c(), out.ctypes.data)
        assert rc == _lib.PR_ERR_INVALID and len(lib.pr_last_error()) > 0, field
    d = _lib.SceneGridDesc.from_buffer_copy(mixed["grid"].desc())
    d.dim[0] = 1 << 20; d.dim[1] = 1 << 10
    assert lib.pr_icp_grid(cloud.data(), 10, C.addressof(d), api.ICPConvergenceCriteria(0.0, 0.0, 1).c(), out.ctypes.data) == _lib.PR_ERR_INVALID


# ---- 5. where the grid is the exact search ----------------------------------------------------------------------------------------------
def test_grid_equals_kdtree_on_cell_centres(gpu):
    """Scene points exactly on the centres of distinct cells, the cloud = those points moved rigidly by less than cell / 4: every grid winner is
    brute force's, and ICP on the grid returns the kd-tree scene's record byte for byte."""
    cell = 1.0 / 128
    lo = np.array([-0.125, -0.125, 0.375])
    i, j = np.meshgrid(np.arange(4, 28), np.arange(4, 28), indexing="ij")
    i, j = i.ravel(), j.ravel()
    zf = 14 + 6 * np.sin(i / 5.0) * np.cos(j / 6.0)
    k = np.rint(zf).astype(int)
    pts = ((np.stack([i, j, k], 1) + 0.5) * cell + lo).astype(F32)
    nrm = _unit(np.stack([-1.2 * np.cos(i / 5.0) * np.cos(j / 6.0), np.sin(i / 5.0) * np.sin(j / 6.0), np.ones(len(i))], 1))
    mdd = 0.05
    scene, grid, desc, pts, nrm = build(pts, nrm, lo, lo + 31.5 * cell, cell, mdd)
    assert desc.dim == (32, 32, 32)
    rng = np.random.default_rng(31)
    cloud = nn_ref.rigid(pts, 0.25, 0.0009, rng)
    assert np.abs(cloud.astype(np.float64) - pts).max() < cell / 4 and np.linalg.norm(cloud.astype(np.float64) - pts, axis=1).max() < cell / 4
    # the premise, on the CPU: every scene point sits in a cell of its own, on its centre; no query has a tie; every cloud point is in its point's cell
    inside, idx = grid_ref.cell_of(pts, desc)
    assert inside.all() and len(np.unique(idx)) == len(pts)
    assert np.array_equal(u32(grid_ref.centres(desc)[idx]), u32(pts))
    bf = nn_ref.BruteForce(cloud, pts, mdd)
    assert (bf.n_ties() == 1).all() and bf.inside.all()
    cin, cidx = grid_ref.cell_of(cloud, desc)
    assert cin.all() and np.array_equal(cidx, idx)
    cp, rec = grid.cell_points().reshape(-1), grid.records()
    winner, valid = grid_ref.associate(cloud, desc, cp, rec)
    _, count, arg = brute_force_first_minimum(cloud, pts, mdd)
    assert valid.all() and (count == 1).all() and np.array_equal(winner, arg.astype(np.uint32))
    # device terms of the two scenes, then the whole loop
    tg = api.debug_contrib29(api.DeviceVector.from_host(cloud.reshape(-1)), grid)
    tn = api.debug_contrib29(api.DeviceVector.from_host(cloud.reshape(-1)), scene)
    assert np.array_equal(u32(tg), u32(tn)) and (tg[:, 28] == 1).all()
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 6)
    dg, dn = api.DeviceVector.from_host(cloud.reshape(-1)), api.DeviceVector.from_host(cloud.reshape(-1))
    rg, rn = api.ICP_Point2Plane(dg, grid, crit), api.ICP_Point2Plane(dn, scene, crit)
    assert u32(rg.transformation_).tobytes() == u32(rn.transformation_).tobytes() and rg.fitness_ == rn.fitness_ == 1.0 and rg.inlier_rmse_ == rn.inlier_rmse_
    assert dg.to_host().tobytes() == dn.to_host().tobytes()
    bg = api.ICP_Point2Plane_batch(api.DeviceVector.from_host(cloud.reshape(-1)), [0, len(cloud)], grid, crit)
    bn = api.ICP_Point2Plane_batch(api.DeviceVector.from_host(cloud.reshape(-1)), [0, len(cloud)], scene, crit)
    assert bg.tobytes() == bn.tobytes()
