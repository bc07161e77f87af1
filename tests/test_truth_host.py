"""The oracle against float64 geometry (tests/truth_ref.py): render, back-projection, the row convention between them, normals, the projective lookup.
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
