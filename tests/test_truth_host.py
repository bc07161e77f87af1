"""The oracle against float64 geometry (tests/truth_ref.py): render, back-projection, the row convention between them, normals, the projective lookup,
and (second half) the refinement loop: per-point terms, pending update, sums, the loop and its fixed point, the fused path.
No GPU.  Every device test of this suite is a parity test against oracle/pose_oracle.c; this file is what makes those meaningful -- it would notice a
misunderstanding that oracle and kernels share -- and it is where the bounds of tests/test_truth_gpu.py are measured (tests/truth_cases.py,
profiles/truth/README.md).  Out of reach of the ray caster and therefore parity-only: triangles with a vertex at or behind z = 1 (dropped from both
sides here; the reference does not clip them, and what it draws of them is a wrap-around, not geometry)."""
import numpy as np
import pytest

import oracle_lib as O
import truth_cases as TC
import truth_ref as T


# ---- render ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,W,H", TC.RENDER_FRAMES)
def test_oracle_render_is_the_ray_cast(seed, W, H):
    s = TC.render_scene(seed, W, H)
    proj = O.compute_proj(s["K"], W, H)
    for i, v in enumerate(s["views"]):
        img = O.render(v["tris"], v["pose"][None], W, H, proj)[0]
        TC.check_render(img, v["z"], v["edge"], f"oracle seed {seed} view {i}")
        for roi in s["rois"]:
            z, edge = T.raycast(v["cam"], s["K"], W, H, roi)
            assert np.allclose(z, TC.window(v["z"], roi), rtol=1e-12, atol=0) and np.allclose(edge, TC.window(v["edge"], roi), rtol=0, atol=1e-12)
            TC.check_render(O.render(v["tris"], v["pose"][None], W, H, proj, roi)[0], z, edge, f"oracle seed {seed} view {i} roi {roi}", cap=False)


# ---- back-projection ------------------------------------------------------------------------------------------------------------------------
def test_oracle_depth2cloud_is_the_back_projection():
    worst = 0.0
    for d, K, stride, tlx, tly in TC.cloud_cases():
        worst = max(worst, TC.check_cloud(O.depth2cloud(d, K, stride, tlx, tly), d, K, stride, tlx, tly, (d.shape, d.dtype, stride, tlx, tly)))
    TC.say(f"depth2cloud oracle: largest relative deviation {worst:.3e}")


# ---- render, then back-project: the row convention -----------------------------------------------------------------------------------------
def test_oracle_cloud_of_a_render_lies_one_row_off_the_mesh():
    s = TC.sloped_scene()
    img = O.render(s["tris"], s["pose"][None], s["W"], s["H"], O.compute_proj(s["K"], s["W"], s["H"]))[0]
    TC.check_row_pin(O.depth2cloud(img, s["K"]), s["cam"], s["K"], s["W"] * s["H"], "oracle sloped", sloped=True)
    r = TC.render_scene(*TC.RENDER_FRAMES[0])
    proj = O.compute_proj(r["K"], r["W"], r["H"])
    for i in (1, 2):
        v = r["views"][i]
        img = O.render(v["tris"], v["pose"][None], r["W"], r["H"], proj)[0]
        TC.check_row_pin(O.depth2cloud(img, r["K"]), v["cam"], r["K"], r["W"] * r["H"], f"oracle random view {i}")
        roi = r["rois"][1]
        TC.check_row_pin(O.depth2cloud(O.render(v["tris"], v["pose"][None], r["W"], r["H"], proj, roi)[0], r["K"], 1, roi[0], roi[1]), v["cam"], r["K"],
                         r["W"] * r["H"], f"oracle random view {i} roi")


def test_cy_plus_one_makes_render_and_back_projection_agree():
    """DESIGN.md section 1 "Image rows": a caller who wants the cloud of a render ON the posed mesh gives compute_proj the principal point (cx, cy + 1)
    and keeps K for everything else -- then the unmoved cloud meets the mesh along its own rays within the render bound."""
    s = TC.sloped_scene()
    K1 = s["K"].copy()
    K1[5] += 1.0
    img = O.render(s["tris"], s["pose"][None], s["W"], s["H"], O.compute_proj(K1, s["W"], s["H"]))[0]
    res, edge = TC.ray_residuals(O.depth2cloud(img, s["K"]), s["cam"], s["K"], 0)
    clear = edge >= TC.EDGE_BAND
    TC.say(f"cy + 1: {len(res)} points, max residual {res[clear].max():.5f} mm")
    assert len(res) > 100 and (~clear).sum() <= TC.EDGE_CAP * s["W"] * s["H"] and res[clear].max() <= TC.RENDER_BOUND


# ---- normals and scene points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_oracle_normals_and_scene_points_on_analytic_surfaces(dtype):
    W, H, K = TC.NORMAL_W, TC.NORMAL_H, TC.NORMAL_K
    worst = 0.0
    for name, d, n_true in TC.normal_cases():
        dd = d.astype(dtype)
        if dtype == np.uint16:
            worst = max(worst, TC.check_normals(O.get_normal(dd, K), d, n_true, f"get_normal {name}"))
        ps = O.ProjScene(dd, K)
        worst = max(worst, TC.check_normals(ps.normal, d, n_true, f"ProjScene {name} {dtype.__name__}"))
        TC.check_scene_points(ps.pcd, d, K, name)
        # the kd-tree scene before its tree reorders it: valid pixels row-major
        pcd, nrm = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
        n = O.lib().po_scene_nn_gather(dd.ctypes.data, int(dtype == np.int32), K, W, H, pcd.reshape(-1), nrm.reshape(-1))
        assert n == int((d > 0).sum())
        TC.check_cloud(pcd[:n], np.clip(d, 0, 65535), K, 1, 0, 0, f"NNScene points {name}")
        assert np.array_equal(nrm[:n], ps.normal.reshape(H, W, 3)[d > 0])
        # ... and as NNScene leaves it, in tree order
        ns = O.NNScene(dd, K)
        pts, nn, mask = TC.nn_points_to_pixels(ns.pcd, ns.normal, K, W, H)
        assert np.array_equal(mask, d > 0)
        TC.check_normals(nn.reshape(-1, 3), d, n_true, f"NNScene {name} {dtype.__name__}")
    TC.say(f"normals oracle {dtype.__name__}: largest angle {worst:.3f} deg")


def test_noise_image_reaches_all_256_subsets_of_the_tap_gates():
    counts = TC.gate_subset_counts(TC.noise_depth())
    TC.say(f"noise image: {int((counts > 0).sum())} of 256 gate subsets, rarest {int(counts.min())} pixels")
    assert (counts > 0).all()
    wide = TC.noise_depth_wide()
    assert (wide < 0).sum() > 100 and (wide > 65535).sum() > 100


# ---- projective lookup ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.LOOKUP_WINDOWS))
def test_oracle_lookup_takes_the_pixel_the_projection_says(name):
    pts, _ = TC.lookup_cloud(name)
    TC.check_lookup(TC.oracle_lookup_rows(name)(pts), name, "oracle")


# =================================================================================================================================================
#  The refinement loop: the oracle's terms, pending update, sums, loop and fused path against the float64 definitions of tests/truth_ref.py.
#  This is where TERM_UNITS_MEASURED ... FUSED_RMSE_REL_MEASURED of tests/truth_cases.py are measured: every test asserts that the figure it
#  finds has not grown past its constant (the checks themselves ask for 1.25 times the constant).
# =================================================================================================================================================
KINDS = ["proj", "nn"]


def scene_arrays(kind, name="whole"):
    """(oracle scene, float64 association, scene points, scene normals) of scene A."""
    s = TC.scene_a_oracle(kind, name)
    assoc = TC.nn_associate(s.pcd) if kind == "nn" else TC.proj_associate(s.pcd, TC.ICP_WINDOWS[name])
    return s, assoc, s.pcd, s.normal


# ---- (a) terms, point by point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("proj", "whole"), ("proj", "cropped"), ("nn", "whole")])
def test_oracle_terms_are_point_to_plane(kind, name):
    cloud, block, _ = TC.cloud_a()
    s, assoc, pcd, nrm = scene_arrays(kind, name)
    truth = TC.truth_terms((kind, name, "a"), cloud, assoc, pcd, nrm)
    worst, share = TC.check_terms(TC.oracle_rows_of(s)(cloud), cloud, block, truth, f"oracle {kind} {name}")
    assert worst <= TC.TERM_UNITS_MEASURED, worst


def test_kdtree_band_holds_every_disagreement():
    """The kd-tree band holds every disagreement of a first pass: on cloud A the oracle's winner (the scene point its walk of the tree ends at) differs
    from brute force in float64 only where the relative gap to the runner-up is below NN_GAP_BAND (on these inputs: nowhere).  How wide the band has to
    be for the LATER passes of a loop is another matter: profiles/truth/README.md "Bands of the loop"."""
    cloud, block, _ = TC.cloud_a()
    s = TC.scene_a_oracle("nn")
    nn = T.nearest(cloud, s.pcd, TC.ICP_MAX_DIST)
    win = np.array([s.query(p)[1] for p in cloud])
    differ = win != nn.winner
    TC.say(f"kd-tree winners on cloud A: {int(differ.sum())} differ from brute force; their gaps {np.sort(nn.margin_gap[differ])[:8]}; smallest gap of an agreeing point "
           f"{nn.margin_gap[~differ].min():.3e}; below the band {int((nn.margin_gap < TC.NN_GAP_BAND).sum())}")
    assert (nn.margin_gap[differ] < TC.NN_GAP_BAND).all()


# ---- (b) the pending update ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_pending_update_moves_the_cloud(kind):
    """O.icp with one iteration returns the cloud moved by its update of pass 0: R p + t with the float64 update of the float64 sums of pass 0."""
    main, _ = TC.cloud_a_main()
    s, assoc, pcd, nrm = scene_arrays(kind)
    t64, _, _, _ = TC.truth_terms((kind, "main"), main, assoc, pcd, nrm)
    E, _, _ = T.float64_truth(t64.sum(0))
    _, passes, moved, _ = O.icp(main, s, (0.0, 0.0, 1), O.SUM_CANONICAL, TC.ICP_PPB)
    assert passes == 2
    worst = TC.check_moved(moved, E, main, f"oracle {kind}")
    assert worst <= TC.MOVED_UNITS_MEASURED, worst
    # ... and the update alone, given as float32 values: what the device's debug entry is asked
    for which, M in TC.given_updates(E).items():
        worst = TC.check_moved(O.transform_cloud(main, M), M, main, f"oracle given {which} ({kind})", TC.MOVED_GIVEN_UNITS_MEASURED)
        assert worst <= TC.MOVED_GIVEN_UNITS_MEASURED, worst


# ---- (c) the 29 sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppb", TC.SUM_PPBS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_sums_are_the_sums_of_the_terms(kind, ppb):
    main, _ = TC.cloud_a_main()
    s, assoc, pcd, nrm = scene_arrays(kind)
    t64, sc, _, margin = TC.truth_terms((kind, "main"), main, assoc, pcd, nrm)
    worst = {}
    for n in TC.SUM_SIZES + (len(main),):
        worst[n] = TC.check_sums(O.sum29(main[:n], s, O.SUM_CANONICAL, ppb), t64[:n], sc[:n], ppb, f"oracle {kind} {n} points")
    seq = float(TC.units(O.sum29(main, s, O.SUM_SEQUENTIAL), t64.sum(0), sc.sum(0)).max())
    TC.say(f"sums oracle {kind} ppb {ppb}: units of 2^-24 of the summed scales per window {({k: round(v, 3) for k, v in worst.items()})}; max {max(worst.values()):.3f}; "
           f"sequential mode on the whole cloud {seq:.1f}; {int((margin < 1).sum())} of {len(main)} points are band members (the truth's decision is used for them too)")
    assert max(worst.values()) <= TC.SUM_UNITS_MEASURED[ppb], worst


# ---- (d) the loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_truth():
    main, _ = TC.cloud_a_main()
    out = {}
    for kind in KINDS:
        s, assoc, pcd, nrm = scene_arrays(kind)
        out[kind] = T.icp(main, assoc, pcd, nrm, max(TC.LOOP_ITERATIONS))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_loop_follows_the_float64_loop_to_the_known_motion(kind, loop_truth):
    main, M = TC.cloud_a_main()
    known = np.linalg.inv(M)
    s = TC.scene_a_oracle(kind)
    for N in TC.LOOP_ITERATIONS:
        rec, passes, _, _ = O.icp(main, s, (0.0, 0.0, N), O.SUM_CANONICAL, TC.ICP_PPB)
        assert passes == N + 1
        traj, rel, fixed = TC.check_loop(rec["T"], rec["fitness"], rec["inlier_rmse"], loop_truth[kind], N, main, known, f"oracle {kind}")
        assert traj <= TC.TRAJ_ADD_MEASURED_MM and rel <= TC.RMSE_REL_MEASURED[N] and fixed <= TC.FIXED_ADD_MEASURED_MM[N], (N, traj, rel, fixed)


# ---- (e) the fused path ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_fused_path_follows_the_float64_loop(kind):
    sb = TC.scene_b()
    proj = O.compute_proj(TC.ICP_K, TC.ICP_W, TC.ICP_H)
    s = (O.NNScene if kind == "nn" else O.ProjScene)(sb["depth"], TC.ICP_K, TC.ICP_MAX_DIST)
    assoc = TC.nn_associate(s.pcd) if kind == "nn" else TC.proj_associate(s.pcd, TC.ICP_WINDOWS["whole"])
    clouds = [O.depth2cloud(O.render(sb["tris"], sb["hyps"][i:i + 1], TC.ICP_W, TC.ICP_H, proj)[0], TC.ICP_K) for i in range(len(sb["hyps"]))]
    truths = [T.icp(cl, assoc, s.pcd, s.normal, TC.FUSED_ITERATIONS) for cl in clouds]
    res, sizes, _ = O.refine_batch(sb["tris"], sb["hyps"], TC.ICP_W, TC.ICP_H, proj, TC.ICP_K, s, (0.0, 0.0, TC.FUSED_ITERATIONS), O.SUM_CANONICAL, TC.ICP_PPB)
    assert np.array_equal(sizes, [len(c) for c in clouds])
    TC.say(f"fused oracle {kind}: cloud sizes {sizes.tolist()}")
    _, worst, worst_rel = TC.check_fused(res, clouds, truths, kind, f"oracle {kind}")
    assert worst <= TC.FUSED_ADD_MEASURED_MM and worst_rel <= TC.FUSED_RMSE_REL_MEASURED, (worst, worst_rel)
    rows0 = [O.sum29(cl, s, O.SUM_CANONICAL, TC.ICP_PPB) for cl in clouds]
    assert TC.check_fused_sums(rows0, clouds, assoc, s.pcd, s.normal, ("fused", kind), f"oracle {kind}") <= TC.SUM_UNITS_MEASURED[TC.ICP_PPB]
