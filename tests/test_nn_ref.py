"""CPU tests of the kd-tree scenes of nn_ref.py: on every family the reference's stackless walk (O.NNScene.query) returns brute force's
winner, and each family has the property it is there for (ties, both sides of the acceptance radius, both sides of the wide walk's frame
test, neighbours within reach).  These are conditions on the INPUTS of test_nn_exact_gpu.py, checked with the reference alone."""
import ctypes as C

import numpy as np
import pytest

import nn_ref as R
import oracle_lib as O
from pose_refine_amd import _lib

DEPTH_FAMILIES = ("F1_clutter", "F2_ties", "F2_near_ties", "F2_ulp_ties", "F3_wide", "F3_97x61", "F3_300x200", "F4_near", "F4_far", "F5_mismatch", "F6_accept")


@pytest.fixture(scope="module")
def families():
    return R.all_depth_families()


def _first_pass(fam, per_cloud, seed, which=None):
    oscene = fam.oracle_scene()
    q = R.sample_queries(fam.clouds, per_cloud, seed, which)
    bf = R.BruteForce(q, oscene.pcd, fam.max_dist)
    return oscene, q, bf


@pytest.mark.parametrize("name", DEPTH_FAMILIES)
def test_stackless_walk_equals_brute_force(families, name):
    """Sampled first-pass queries of every cloud: the oracle's walk returns the minimum distance, a point of the tie set, and a
    correspondence exactly when the minimum is below accept."""
    fam = families[name]
    which = (0, 3, 5) if name == "F1_clutter" else None
    oscene, q, bf = _first_pass(fam, 400 if name == "F1_clutter" else 300, 5, which)
    assert R.check_oracle_against_brute_force(oscene, q, bf) == len(q) > 0
    ulps = R.gap_ulps(bf)
    print(f"{name}: {len(oscene.pcd)} scene points, {len(q)} queries, inside {bf.inside.mean():.3f}, exact ties {(bf.n_ties() > 1).sum()}, "
          f"near ties (<= 4 ulp) {((ulps > 0) & (ulps <= 4)).sum()}")


@pytest.mark.parametrize("name", ("F1_clutter", "F3_wide", "F6_accept", "F4_far"))
def test_uint16_and_int32_images_make_the_same_scene(families, name):
    a = families[name].oracle_scene()
    b = families[name].as_dtype(np.uint16).oracle_scene()
    assert a.pcd.tobytes() == b.pcd.tobytes() and a.normal.tobytes() == b.normal.tobytes() and a.nodes.tobytes() == b.nodes.tobytes()


def test_f2_queries_are_exact_ties(families):
    _, _, bf = _first_pass(families["F2_ties"], 300, 7)
    frac = (bf.n_ties() > 1).mean()
    print("F2 exact ties:", frac)
    assert frac >= 0.9


def test_f2_near_ties_are_near_but_not_exact(families):
    """The lines moved 2 um: most queries now have ONE nearest point, with a runner-up a hair further."""
    _, _, bf = _first_pass(families["F2_near_ties"], 300, 7)
    unique = bf.n_ties() == 1
    rel = bf.gap / bf.d2
    print("F2 near: unique", unique.mean(), "median relative gap", float(np.median(rel[unique])))
    assert unique.mean() >= 0.9
    assert np.median(rel[unique]) < 1e-2


def test_f2_ulp_ties_differ_by_a_few_ulps(families):
    """The lines moved 0.5 nm: the two mirror-image candidates are no longer tied, but their squared distances differ by a few ulps."""
    _, _, bf = _first_pass(families["F2_ulp_ties"], 300, 7)
    unique = bf.n_ties() == 1
    ulps = R.gap_ulps(bf)
    print("F2 ulp: unique", unique.mean(), "gap in ulps: median", float(np.median(ulps[unique])), "max", float(ulps[unique].max()))
    assert unique.mean() >= 0.9
    assert np.percentile(ulps[unique], 90) <= 4


def test_f6_distances_fall_on_both_sides_of_accept(families):
    _, _, bf = _first_pass(families["F6_accept"], 1000, 9)
    print("F6 inside:", int(bf.inside.sum()), "outside:", int((~bf.inside).sum()))
    assert bf.inside.sum() >= 50 and (~bf.inside).sum() >= 50
    assert np.all(np.abs(bf.d2.astype(np.float64) - float(bf.accept)) < 1e-6)      # every query is near the boundary


@pytest.mark.parametrize("name", ("F1_clutter", "F3_wide", "F3_97x61", "F3_300x200", "F5_mismatch"))
def test_first_pass_queries_mostly_have_a_neighbour(families, name):
    _, _, bf = _first_pass(families[name], 300, 11)
    print(name, "inside:", bf.inside.mean())
    assert bf.inside.mean() >= 0.5


def test_f5_scene_points_own_distinct_pixels_under_both_cameras(families):
    """The pixel grid is usable only when every scene point projects into a cell of its own: F5's scene keeps clear of the border so that
    this holds under the fused camera K' as well as under K."""
    fam = families["F5_mismatch"]
    pcd = fam.oracle_scene().pcd
    for K in (fam.K, fam.K_fused):
        # grid_project (nn_query.h), float32: cells centred on the pixels
        u = np.floor(pcd[:, 0] / pcd[:, 2] * K[0] + K[2] + np.float32(0.5)).astype(np.int64)
        v = np.floor(pcd[:, 1] / pcd[:, 2] * K[4] + K[5] + np.float32(0.5)).astype(np.int64)
        assert u.min() >= 0 and u.max() < fam.W and v.min() >= 0 and v.max() < fam.H
        assert len(np.unique(v * fam.W + u)) == len(pcd)


@pytest.mark.parametrize("kind", R.DEGENERATE)
def test_degenerate_scenes(kind):
    """Camera-less scenes: pr_kdtree_build and the oracle's po_kd_build give byte-equal nodes (and reorder the points alike), and the
    stackless walk equals brute force on sampled queries."""
    fam = R.degenerate(kind)
    pts, nrm = fam.pts.copy(), fam.nrm.copy()
    nodes = np.zeros(2 * len(pts) + 1, _lib.KDNODE); cnt = C.c_uint32()
    _lib.check(_lib.load().pr_kdtree_build(pts.ctypes.data, nrm.ctypes.data, len(pts), fam.max_leaf, nodes.ctypes.data, len(nodes), C.byref(cnt)))
    oscene = fam.oracle_scene()
    assert oscene.nodes.tobytes() == nodes[:cnt.value].tobytes()
    assert oscene.pcd.tobytes() == pts.tobytes() and oscene.normal.tobytes() == nrm.tobytes()
    wrapped = O.NNScene.from_points(pts, nrm, fam.max_dist, nodes=nodes[:cnt.value])
    q = R.sample_queries(fam.clouds, 300, 13)
    bf = R.BruteForce(q, oscene.pcd, fam.max_dist)
    assert R.check_oracle_against_brute_force(oscene, q, bf) == len(q)
    assert R.check_oracle_against_brute_force(wrapped, q[:50], R.BruteForce(q[:50], pts, fam.max_dist)) == 50
    if kind == "repeated":
        assert np.all(bf.n_ties() == 500)
    assert bf.inside.mean() >= 0.5


def test_far_scenes_straddle_the_wide_frame_test():
    """info[20] (nn_frame_kernel, restated in float32): the 0.2 m cube 40 m out may use the wide walk's integer box test, 60 m out not."""
    got = {k: R.wide_frame_ok(R.degenerate(k).oracle_scene().nodes, 0.1) for k in ("far40", "far60")}
    assert got == {"far40": True, "far60": False}
    assert R.wide_frame_ok(R.degenerate("coplanar").oracle_scene().nodes, 0.1)


def test_vine_is_a_consistent_tree_deeper_than_any_stack():
    """The hand-made vine: 127 nodes over 64 leaves of 1 to 10 points; links, point ranges and boxes agree; left_max <= split <= right_min at
    every internal node, with equality at the tie levels; one point is held twice; its depth, from the links, is beyond the 24-entry stacks."""
    fam = R.vine()
    nodes, pts = fam.nodes, fam.pts
    assert len(nodes) == 2 * R.VINE_LEAVES - 1 == 127 and R.tree_depth(nodes) == R.VINE_LEAVES - 1 > 24
    leaf = nodes["child1"] < 0
    assert leaf.sum() == R.VINE_LEAVES and np.array_equal(leaf, nodes["child2"] < 0)
    sizes = (nodes["right"] - nodes["left"])[leaf]
    assert sizes.min() == 1 and sizes.max() == 10 and sizes.sum() == len(pts) == nodes[0]["right"] and nodes[0]["left"] == 0 and nodes[0]["parent"] == -1
    covered = np.zeros(len(pts), np.int64)
    for nd in nodes[leaf]:
        covered[nd["left"]:nd["right"]] += 1
    assert (covered == 1).all()                                     # the leaves tile the point array
    ties = 0
    for i, nd in enumerate(nodes):
        q = pts[nd["left"]:nd["right"]]
        assert np.array_equal(nd["bbox"], np.stack([q.min(0), q.max(0)], 1).reshape(-1)), i
        if leaf[i]:
            continue
        a, b, d = nodes[nd["child1"]], nodes[nd["child2"]], int(nd["split_dim"])
        assert nd["child2"] == nd["child1"] + 1 > i and a["parent"] == b["parent"] == i
        assert (a["left"], a["right"], b["right"]) == (nd["left"], b["left"], nd["right"]) and a["left"] < a["right"] < b["right"]
        assert leaf[nd["child1"]] or leaf[nd["child2"]]            # one leaf is split off per level
        left_max, right_min = pts[a["left"]:a["right"], d].max(), pts[b["left"]:b["right"], d].min()
        assert left_max <= nd["split_v"] <= right_min, (i, left_max, nd["split_v"], right_min)
        ties += int(left_max == right_min)
    assert ties == len(R.VINE_TIE_LEVELS)
    assert len(np.unique(pts, axis=0)) == len(pts) - 1              # the duplicate pair


def test_vine_walk_equals_brute_force():
    """The oracle's stackless walk over the vine returns brute force's distance, a point of its tie set and the same acceptance, on the
    vine's 2000 queries and on the scene points themselves (distance 0: the duplicate pair ties)."""
    fam = R.vine()
    oscene = fam.oracle_scene()
    assert oscene.nodes.tobytes() == fam.nodes.tobytes() and oscene.pcd.tobytes() == fam.pts.tobytes()
    q = fam.clouds[0]
    assert len(q) == 2000
    bf = R.BruteForce(q, oscene.pcd, fam.max_dist)
    assert R.check_oracle_against_brute_force(oscene, q, bf) == len(q) > 0
    assert bf.inside.mean() >= 0.5
    own = R.BruteForce(fam.pts, oscene.pcd, fam.max_dist)
    assert R.check_oracle_against_brute_force(oscene, fam.pts, own) == len(fam.pts)
    assert (own.d2 == 0).all() and (own.n_ties() > 1).sum() == 2


@pytest.mark.parametrize("max_dist", [0.1, 0.003])
def test_inside_count_is_brute_forces_count(max_dist):
    """R.inside_count (the strided shortcut the GPU tests count first-pass inliers with) equals BruteForce's count, with every query inside
    and with queries on both sides of the radius."""
    fam = R.degenerate("coplanar")
    q = fam.clouds[0]
    bf = R.BruteForce(q, fam.pts, max_dist)
    assert R.inside_count(q, fam.pts, max_dist) == int(bf.inside.sum())
    if max_dist < 0.01:
        assert 50 < bf.inside.sum() < len(q) - 50
