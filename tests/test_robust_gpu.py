"""GPU tests (-m gpu) of the robust ICP pass (pr_robust, include/pose_refine.h) against tests/robust_ref.py, bit for bit: the weighted per-point
terms and weights (pr_debug_robust_terms), the 29 sums of every pass (pr_icp_batch_robust under pr_debug_trace_sums), the device solve against
the host solve, the identity w == 1 on every scene kind, the fused path and its two-level anneal, a mixed batch, and the kd-tree options.

Correspondences: for the closest-point grid the reference is numpy throughout (grid_ref.associate).  For projective and kd-tree scenes the
reference takes the library's own correspondences -- corr_host of a PR_ROBUST_NONE call to pr_debug_robust_terms on the reference's current
cloud -- after the per-point test has tied them to the tested path: plain terms formed from corr_host with grid_ref.terms29's arithmetic equal
pr_debug_contrib29's rows bit for bit."""
import numpy as np
import pytest

import grid_ref
import oracle_lib as O
import pyramid_ref
import robust_ref as R
import truth_cases as TC
from gpu_common import TOL_T
from pass_sums_ref import odd_start_order, u32, window
from pose_refine_amd import api
from test_pass_sums_gpu import options, ragged, traced, written_passes

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = (R.HUBER, R.TUKEY, R.CAUCHY)
NAMES = {R.NONE: "none", R.HUBER: "huber", R.TUKEY: "tukey", R.CAUCHY: "cauchy"}
C_PASS = 0.005                                                   # 5 mm: the scenario's first-pass residuals spread over several centimetres
CRIT_PASS = (0.0, 0.0, 4)
SIZES, NN_SIZES = (1, 64, 65, 257, 1025, 3073, 6145), (1, 65, 1025, 3073)


def dv(cloud):
    return api.DeviceVector.from_host(np.ascontiguousarray(cloud, F32).reshape(-1))


def lib_associate(scene, packed):
    """associate(cloud) from the library's own correspondences (corr_host of a PR_ROBUST_NONE call)."""
    none = api.Robust(api.ROBUST_NONE)

    def associate(cloud):
        _, corr = api.debug_robust_terms(dv(cloud), scene, none, packed=packed)
        return corr[:, 0:3].copy(), corr[:, 4:7].copy(), corr[:, 3] == 1.0
    return associate


class Kit:
    """One scene as the tests need it: the device scene, whether the packed record is asked for, and associate(cloud) of the reference."""

    def __init__(self, name, scene, packed=False, grid_host=None):
        self.name, self.scene, self.packed = name, scene, packed
        self.associate = R.grid_associate(*grid_host) if grid_host else lib_associate(scene, packed)
        self.numpy_only = grid_host is not None


def grid_of(nn):
    g = api.Scene_grid.from_scene_nn(nn, 0.004)
    return g, (grid_ref.from_ctypes(g.desc()), g.cell_points().reshape(-1), g.records())


@pytest.fixture(scope="module")
def kits(gpu, gscenes):
    grid, host = grid_of(gscenes["nn"])
    return {"proj": Kit("proj", gscenes["proj"]), "packed": Kit("packed", gscenes["proj"], packed=True), "nn": Kit("nn", gscenes["nn"]),
            "grid": Kit("grid", grid, grid_host=host)}


def small_update():
    """A pending update: 0.4 degrees about (2, -1, 3) and 1.5 mm, float32."""
    ax = np.array([2.0, -1.0, 3.0]); ax /= np.linalg.norm(ax)
    th = np.deg2rad(0.4)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    E[:3, 3] = (0.001, -0.0005, 0.001)
    return E.astype(F32)


# ---- 1. per-point terms and weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_update", [False, True], ids=["no-update", "update16"])
@pytest.mark.parametrize("name", ["proj", "packed", "nn", "grid"])
def test_per_point_terms_and_weights(kits, scenario, name, with_update):
    """pr_debug_robust_terms for windows of 1, 65, 257 and 1025 points and the three kinds.  c lies halfway between the two middle values of the
    window's sorted |r| (valid correspondences), so both sides of c are populated (asserted) and no |r| EQUALS c -- at |r| == c exactly Tukey's
    q = (r * inv_c)^2 is below 1 whenever c * inv_c rounds below 1, which the definition allows and "zero at and beyond c" does not see.  A
    window of ONE point cannot straddle a scale, so it runs twice, with c at half and at twice its |r|, and the two runs together cover both
    sides (asserted)."""
    kit = kits[name]
    upd = small_update() if with_update else None
    none = api.Robust(api.ROBUST_NONE)
    for n in (1, 65, 257, 1025):
        cloud = window(scenario["cloud"], n)
        moved = grid_ref.transform(cloud, upd) if with_update else np.ascontiguousarray(cloud, F32)
        what = (name, n, with_update)
        # the correspondences of the tested path, tied to pr_debug_contrib29
        d0 = dv(cloud)
        terms0, corr0 = api.debug_robust_terms(d0, kit.scene, none, update=upd, packed=kit.packed)
        assert np.array_equal(u32(d0.to_host().reshape(-1, 3)), u32(moved)), what            # the update went into the cloud, in the pass' arithmetic
        plain = api.debug_contrib29(dv(cloud), kit.scene, update=upd, packed=kit.packed)
        assert terms0.tobytes() == plain.tobytes(), what
        valid = corr0[:, 3] == 1.0
        assert valid.any() and set(np.unique(corr0[:, 3])) <= {0.0, 1.0}, what
        assert (corr0[valid, 7] == 1.0).all() and not u32(corr0[~valid]).any(), what
        corr = (corr0[:, 0:3], corr0[:, 4:7], valid)
        assert np.array_equal(u32(R.plain_terms29(moved, corr)), u32(plain)), what
        if kit.numpy_only:                                         # the grid: numpy finds the same correspondences
            d, nr, v = kit.associate(moved)
            assert np.array_equal(v, valid) and np.array_equal(u32(d[v]), u32(corr[0][v])) and np.array_equal(u32(nr[v]), u32(corr[1][v])), what
        a = np.abs(R.residuals(moved, corr)[valid])
        mid = np.sort(a.astype(np.float64))[len(a) // 2 - 1:len(a) // 2 + 1]
        scales = [float(mid.mean())] if n > 1 else [float(a[0]) * 0.5, float(a[0]) * 2.0]
        assert n == 1 or mid[0] < F32(scales[0]) < mid[1], what
        for kind in KINDS:
            below = above = False
            for c in scales:
                rb = api.Robust(kind, c)
                below |= bool((a < rb.c).any()); above |= bool((a > rb.c).any())
                got, gcorr = api.debug_robust_terms(dv(cloud), kit.scene, rb, update=upd, packed=kit.packed)
                want, w = R.weighted_terms29(moved, corr, rb)
                assert np.array_equal(u32(gcorr[:, :7]), u32(corr0[:, :7])), what + (NAMES[kind],)
                assert np.array_equal(u32(gcorr[:, 7]), u32(w)), what + (NAMES[kind], "weights")
                assert np.array_equal(u32(got), u32(want)), what + (NAMES[kind], "terms", int((u32(got) != u32(want)).sum()))
                assert np.array_equal(u32(got[:, 27:]), u32(plain[:, 27:])), what
                if kind == R.TUKEY:
                    out = valid & (np.abs(R.residuals(moved, corr)) >= rb.c)
                    assert not u32(got[out, :27]).any() and (got[out, 28] == 1.0).all() and np.array_equal(u32(got[out, 27]), u32(plain[out, 27])), what
                    if n > 1:
                        assert out.any(), what
                no_corr, _ = api.debug_robust_terms(dv(cloud), kit.scene, rb, update=upd, packed=kit.packed, want_corr=False)
                assert no_corr.tobytes() == got.tobytes(), what
            assert below and above, what + (NAMES[kind], "both sides of c")


# ---- 2. pass sums ---------------------------------------------------------------------------------------------------------------------------
def robust_batch(flat, offs, scene, crit, rb):
    return api.ICP_Point2Plane_batch(dv(flat), offs, scene, api.ICPConvergenceCriteria(*crit), robust=rb)


_loops = {}


def ref_loop(kit, cloud, rb, crit, ppb):
    """robust_ref.loop, computed once per (scene, cloud, descriptor, criteria, tree) and shared read-only."""
    key = (kit.name, np.ascontiguousarray(cloud, F32).tobytes(), rb.kind, float(rb.c), tuple(crit), int(ppb))
    if key not in _loops:
        T, rmse, fitness, rows = R.loop(cloud, kit.associate, rb, crit, ppb)
        rows.setflags(write=False)
        _loops[key] = (T, rmse, fitness, rows)
    return _loops[key]


def assert_batch(kit, parts, res, rows, rb, crit, ppb, what):
    """Every recorded row against robust_ref.loop's, bit for bit; rows that must not be written are NaN; the records as test_pass_sums_gpu.py
    compares them (scores exact, transforms within 1e-4 for clouds whose system has full rank)."""
    want = np.full(rows.shape, np.nan, F32)
    passes = []
    for i, cl in enumerate(parts):
        T, rmse, fitness, tr = ref_loop(kit, cl, rb, crit, ppb)
        want[:len(tr), i] = tr
        passes.append(len(tr))
    bad = [(it, i, len(parts[i]), int((u32(rows[it, i]) != u32(want[it, i])).sum())) for it in range(rows.shape[0]) for i in range(len(parts))
           if not np.array_equal(u32(rows[it, i]), u32(want[it, i]))]
    assert not bad, (what, "(pass, cloud, points, differing columns)", sorted(bad)[:12])
    assert np.array_equal(written_passes(rows), passes), what
    for i, cl in enumerate(parts):
        T, rmse, fitness, _ = ref_loop(kit, cl, rb, crit, ppb)
        assert res[i]["fitness"] == F32(fitness) and res[i]["inlier_rmse"] == F32(rmse), (what, i, len(cl))
        if len(cl) >= 63:
            assert np.allclose(res[i]["T"], T, rtol=0, atol=TOL_T), (what, i, len(cl))
    return passes


@pytest.mark.parametrize("kind", [R.HUBER, R.TUKEY], ids=["huber", "tukey"])
@pytest.mark.parametrize("ppb", [1024, 3072])
@pytest.mark.parametrize("name", ["proj", "grid", "nn"])
def test_pass_sums_every_pass(kits, scenario, name, ppb, kind):
    """pr_icp_batch_robust under pr_debug_trace_sums, host solve, five passes: every row is robust_ref.loop's.  The batch starts most clouds at
    odd point indices; 1024 and 3072 points per workgroup put one to seven workgroups on a cloud."""
    kit = kits[name]
    rb = api.Robust(kind, C_PASS)
    parts = [window(scenario["cloud"], n) for n in odd_start_order(list(NN_SIZES if name == "nn" else SIZES))]
    flat, offs = ragged(parts)
    with options(points_per_block=ppb):
        res, rows = traced(len(parts), CRIT_PASS[2] + 2, lambda: robust_batch(flat, offs, kit.scene, CRIT_PASS, rb))
        untraced = robust_batch(flat, offs, kit.scene, CRIT_PASS, rb)
        plain = api.ICP_Point2Plane_batch(dv(flat), offs, kit.scene, api.ICPConvergenceCriteria(*CRIT_PASS))
    assert res.tobytes() == untraced.tobytes()
    assert res.tobytes() != plain.tobytes()                        # the weight does something at 5 mm
    passes = assert_batch(kit, parts, res, rows, rb, CRIT_PASS, ppb, (name, ppb, NAMES[kind]))
    assert max(passes) == CRIT_PASS[2] + 1 and np.isnan(rows[CRIT_PASS[2] + 1]).all()      # all five passes ran, the spare one was left alone
    print((name, ppb, NAMES[kind]), "passes per cloud", passes)


# ---- 3. device solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.HUBER, R.TUKEY], ids=["huber", "tukey"])
@pytest.mark.parametrize("name", ["proj", "grid", "nn"])
def test_device_solve_gives_the_host_solve_records(kits, scenario, name, kind):
    """The same batch with the solve on the device, as launches of its own and fused into the pass tail, with and without the captured graph:
    the records of the host-solve call, byte for byte."""
    kit = kits[name]
    rb = api.Robust(kind, C_PASS)
    parts = [window(scenario["cloud"], n) for n in odd_start_order(list(NN_SIZES if name == "nn" else SIZES))]
    flat, offs = ragged(parts)
    host = robust_batch(flat, offs, kit.scene, CRIT_PASS, rb)
    for fused in (0, 1):
        for graph in (1, 0):
            with options(solve=api.SOLVE_DEVICE, fused_solve=fused, graph=graph):
                dev = robust_batch(flat, offs, kit.scene, CRIT_PASS, rb)
            diff = [(i, len(parts[i])) for i in range(len(parts)) if dev[i].tobytes() != host[i].tobytes()]
            assert not diff, (name, NAMES[kind], f"fused_solve {fused} graph {graph}", "(cloud, points)", diff)


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_b(gpu):
    """The small mesh and frame of test_truth_gpu.py's fused test (truth_cases.scene_b) with its three scenes."""
    sb = TC.scene_b()
    W, H, K = TC.ICP_W, TC.ICP_H, TC.ICP_K
    d = np.array(sb["depth"], np.int32)
    proj_scene = api.Scene_projective().init_Scene_projective_cuda(d, K, W, H, TC.ICP_MAX_DIST)
    nn = api.Scene_nn().init_Scene_nn_cuda(d, K, max_dist_diff=TC.ICP_MAX_DIST) if W == 640 and H == 480 else \
        api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(d.reshape(-1)), K, W, H, max_dist_diff=TC.ICP_MAX_DIST)
    grid, host = grid_of(nn)
    projection = api.compute_proj(K, W, H)
    kits = {"proj": Kit("b-proj", proj_scene, packed=True), "nn": Kit("b-nn", nn), "grid": Kit("b-grid", grid, grid_host=host)}
    return dict(sb=sb, W=W, H=H, K=K, projection=projection, model=api.Model(tris=sb["tris"]), kits=kits, hyps=sb["hyps"])


DESCRIPTORS_ID = [(R.NONE, 0.0), (R.HUBER, 1.0e6), (R.TUKEY, 1.0e6), (R.CAUCHY, 1.0e6)]


@pytest.mark.parametrize("name", ["proj", "nn", "grid"])
def test_identity_bare_clouds(kits, scenario, name):
    """w == 1.0f for every correspondence (c = 1e6, or PR_ROBUST_NONE): pr_icp_batch_robust returns pr_icp_batch's bytes, under both solves."""
    kit = kits[name]
    parts = [window(scenario["cloud"], n) for n in odd_start_order(list(NN_SIZES))]
    flat, offs = ragged(parts)
    for solve in (api.SOLVE_HOST, api.SOLVE_DEVICE):
        with options(solve=solve):
            plain = api.ICP_Point2Plane_batch(dv(flat), offs, kit.scene, api.ICPConvergenceCriteria(*CRIT_PASS))
            for kind, c in DESCRIPTORS_ID:
                got = robust_batch(flat, offs, kit.scene, CRIT_PASS, api.Robust(kind, c))
                assert got.tobytes() == plain.tobytes(), (name, solve, NAMES[kind])


@pytest.mark.parametrize("name", ["proj", "nn", "grid"])
def test_identity_fused_path(scene_b, name):
    """A one-level stride-1 pr_refine_pyramid_robust returns pr_refine_batch_roi's bytes on the eight hypotheses of scene B."""
    b, kit = scene_b, scene_b["kits"][name]
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 6)
    for solve in (api.SOLVE_HOST, api.SOLVE_DEVICE):
        with options(solve=solve):
            plain, psizes = api.refine_batch(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, crit, roi=(0, 0, 0, 0))
            for kind, c in DESCRIPTORS_ID:
                got, sizes = api.refine_batch(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, crit, roi=(0, 0, 0, 0), robust=api.Robust(kind, c))
                assert got.tobytes() == plain.tobytes() and np.array_equal(sizes, psizes), (name, solve, NAMES[kind])


# ---- 5. fused path ------------------------------------------------------------------------------------------------------------------------------
def oracle_level_clouds(b, strides):
    out = []
    for i in range(len(b["hyps"])):
        depth = O.render(b["sb"]["tris"], b["hyps"][i:i + 1], b["W"], b["H"], b["projection"])[0]
        c1, keep = pyramid_ref.level_clouds(depth, b["K"], strides)
        out.append([np.ascontiguousarray(c1[k]) for k in keep])
    return out


def assert_record(rec, T, rmse, fitness, n, what):
    assert rec["fitness"] == F32(fitness) and rec["inlier_rmse"] == F32(rmse), what
    if n >= 63:
        assert np.allclose(rec["T"], T, rtol=0, atol=TOL_T), what


@pytest.mark.parametrize("kind", [R.HUBER, R.TUKEY], ids=["huber", "tukey"])
@pytest.mark.parametrize("name", ["grid", "proj", "nn"])
def test_fused_path_follows_the_reference(scene_b, name, kind):
    """refine_batch(robust=...) -- pr_refine_pyramid_robust, one level of stride 1 -- on scene B, seven passes: cloud sizes and records against
    robust_ref.loop on the level clouds pyramid_ref.level_clouds makes from the oracle's render."""
    b, kit = scene_b, scene_b["kits"][name]
    crit = (0.0, 0.0, 6)
    rb = api.Robust(kind, 0.003)
    clouds = [lv[0] for lv in oracle_level_clouds(b, [1])]
    ppb = api.get_option("points_per_block")
    res, sizes = api.refine_batch(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, api.ICPConvergenceCriteria(*crit), robust=rb)
    assert np.array_equal(sizes, [len(c) for c in clouds])
    for i, cl in enumerate(clouds):
        T, rmse, fitness, rows = ref_loop(kit, cl, rb, crit, ppb)
        assert len(rows) == crit[2] + 1
        assert_record(res[i], T, rmse, fitness, len(cl), (name, NAMES[kind], i))
    with options(solve=api.SOLVE_DEVICE):
        dev, _ = api.refine_batch(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, api.ICPConvergenceCriteria(*crit), robust=rb)
    assert dev.tobytes() == res.tobytes(), (name, NAMES[kind], "device solve")


@pytest.mark.parametrize("name", ["grid", "proj"])
def test_two_level_anneal_follows_the_reference(scene_b, name):
    """Stride 2 with a wide Huber scale, then stride 1 with a narrow Tukey scale: the reference composed level by level as pyramid_ref.refine_pyramid
    composes it (the level cloud moved by the accumulated transform, T_acc = T_l * T_acc)."""
    b, kit = scene_b, scene_b["kits"][name]
    levels = [(2, (0.0, 0.0, 4)), (1, (0.0, 0.0, 3))]
    table = [api.Robust(R.HUBER, 0.010), api.Robust(R.TUKEY, 0.004)]
    ppb = api.get_option("points_per_block")
    res, lres, lsizes = api.refine_pyramid(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, levels=levels, return_levels=True, robust=table)
    eye = np.eye(4, dtype=F32).reshape(16)
    for i, lv in enumerate(oracle_level_clouds(b, [2, 1])):
        t_acc = eye.copy()
        for l, (cloud, (_, crit), rb) in enumerate(zip(lv, levels, table)):
            if l > 0:
                cloud = pyramid_ref.transform_cloud(cloud, t_acc)
            assert lsizes[l, i] == len(cloud) and len(cloud) > 0
            T, rmse, fitness, _ = ref_loop(kit, cloud, rb, crit, ppb)
            assert_record(lres[l, i], T, rmse, fitness, len(cloud), (name, i, l))
            t_acc = pyramid_ref.mat4_mul(lres[l, i]["T"], t_acc)     # (the library's own level record: every level is compared on its own)
        assert np.array_equal(u32(res[i]["T"]), u32(t_acc)), (name, i)
        assert res[i]["fitness"] == lres[1, i]["fitness"] and res[i]["inlier_rmse"] == lres[1, i]["inlier_rmse"]
    one = api.refine_pyramid(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, levels=levels, robust=table[0])[0]
    same = api.refine_pyramid(b["model"], b["hyps"], b["W"], b["H"], b["projection"], b["K"], kit.scene, levels=levels, robust=[table[0], table[0]])[0]
    assert one.tobytes() == same.tobytes() and one.tobytes() != res.tobytes()      # n_robust == 1 is the descriptor on every level


# ---- 6. mixed batch, options ----------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_the_single_mesh_calls(scene_b):
    """Two meshes x four hypotheses through pr_refine_pyramid_robust_multi: each record is the single-mesh robust call's, byte for byte."""
    b, kit = scene_b, scene_b["kits"]["proj"]
    small = api.Model(tris=np.ascontiguousarray(b["sb"]["tris"] * F32(0.9)))
    meshes = [b["model"], small]
    idx = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.uint32)
    levels = [(2, (0.0, 0.0, 3)), (1, (0.0, 0.0, 3))]
    table = [api.Robust(R.HUBER, 0.008), api.Robust(R.CAUCHY, 0.003)]
    args = (b["W"], b["H"], b["projection"], b["K"], kit.scene)
    res, lres, lsizes = api.refine_pyramid_multi(meshes, idx, b["hyps"], *args, levels=levels, return_levels=True, robust=table)
    for m in (0, 1):
        sel = np.flatnonzero(idx == m)
        r1, l1, s1 = api.refine_pyramid(meshes[m], b["hyps"][sel], *args, levels=levels, return_levels=True, robust=table)
        assert res[sel].tobytes() == r1.tobytes() and lres[:, sel].tobytes() == l1.tobytes() and np.array_equal(lsizes[:, sel], s1), m
    flat, fsizes = api.refine_batch_multi(meshes, idx, b["hyps"], *args, api.ICPConvergenceCriteria(0.0, 0.0, 3), robust=table[0])
    for m in (0, 1):
        sel = np.flatnonzero(idx == m)
        r1, s1 = api.refine_batch(meshes[m], b["hyps"][sel], *args, api.ICPConvergenceCriteria(0.0, 0.0, 3), robust=table[0])
        assert flat[sel].tobytes() == r1.tobytes() and np.array_equal(fsizes[sel], s1), m


def test_kdtree_options_do_not_change_a_byte(kits, scenario):
    """A robust call on a kd-tree scene takes the split route whenever the scene has compact records; without them (nn_compact 0) it searches in
    the pass.  Either way: the bytes of the default options."""
    rb = api.Robust(R.HUBER, C_PASS)
    parts = [window(scenario["cloud"], n) for n in odd_start_order(list(NN_SIZES))]
    flat, offs = ragged(parts)
    default = robust_batch(flat, offs, kits["nn"].scene, CRIT_PASS, rb)
    for cfg in (dict(nn_split=0, nn_compact=0), dict(nn_split=0), dict(nn_split=0, nn_stack=0)):
        with options(**cfg):
            got = robust_batch(flat, offs, kits["nn"].scene, CRIT_PASS, rb)
        assert got.tobytes() == default.tobytes(), cfg
