"""GPU tests (-m gpu) of the kd-tree correspondence search on the hard scenes of nn_ref.py, pass by pass.

(a) Bare ICP with zero criteria and max_iteration = k: the cloud comes back at the positions of its last pass, so the fitness and rmse the
    product reports must be those of the reference's sums over the RETURNED cloud, bit for bit -- one wrong winner whose squared residual
    differs from the right one's by more than half an ulp of the sum shows.  The oracle's query is held to brute force on a sample of it.
(b) Every search form (per-lane stacks with compact or exact records, seeded or not, wide task walk, split or fused search, pixel window on
    or off) against the reference-style stackless walk, bit for bit: bare calls, fused batches, an asynchronous pair, a mismatched camera.
(c) The paths the exactness arguments guard are taken: queries settled by the pixel window, handed to the tree, and kept without a search.
"""
import contextlib

import numpy as np
import pytest

import nn_ref as R
import oracle_lib as O
from pose_refine_amd import api, synth
from gpu_common import make_scene

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, 4, 8, 30, 90)
OPTS = ("nn_stack", "nn_compact", "nn_seed", "nn_wide", "nn_split", "nn_grid")
# (stack, compact, seed, wide, split): the combinations of the existing kd-tree tests; the reference form is the stackless walk
FORMS = ((1, 1, 1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 0, 0), (1, 1, 0, 1, 1), (1, 1, 0, 0, 1), (1, 0, 0, 0, 1))
REF_FORM = (0, 0, 0, 0, 1, 1)
VARIANTS = [f + (g,) for f in FORMS for g in (1, 0)]
U16_TWINS = ("F1_clutter", "F3_wide", "F4_far", "F6_accept")


@contextlib.contextmanager
def options(**kw):
    old = {k: api.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            api.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            api.set_option(k, v)


def form(values):
    return dict(zip(OPTS, values))


@pytest.fixture(scope="module")
def fams():
    return R.all_depth_families()


class Case:
    """A family with its product scene and the oracle's, checked to hold the same points and tree."""

    def __init__(self, fam, dtype=None):
        self.fam = fam
        if fam.depth is None:
            pts, nrm = fam.pts.copy(), fam.nrm.copy()
            self.scene = make_scene(pts, nrm, fam.max_leaf, max_dist=fam.max_dist)     # pr_kdtree_build reorders pts / nrm in place
            self.oscene = O.NNScene.from_points(pts, nrm, fam.max_dist, nodes=self.scene.nodes_host)
            assert self.oscene.nodes.tobytes() == fam.oracle_scene().nodes.tobytes()
            self.name = fam.name
            return
        self.oscene = fam.oracle_scene()
        depth = fam.depth.astype(dtype or np.int32)
        if dtype == np.uint16:
            self.scene = api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(depth.reshape(-1), depth.dtype), fam.K, fam.W, fam.H,
                                                             max_dist_diff=fam.max_dist)
            n, m = len(self.oscene.pcd), len(self.oscene.nodes)
            assert (self.scene._n_points, self.scene._n_nodes) == (n, m)
            assert self.scene.pcd_buffer.to_host()[:3 * n].tobytes() == self.oscene.pcd.tobytes()
            assert self.scene.nodes.to_host()[:m].tobytes() == self.oscene.nodes.tobytes()
            self.name = fam.name + "_u16"
        else:
            self.scene = api.Scene_nn().init_Scene_nn_cuda(depth, fam.K, max_dist_diff=fam.max_dist)
            assert self.scene.pcd_host.tobytes() == self.oscene.pcd.tobytes() and self.scene.nodes_host.tobytes() == self.oscene.nodes.tobytes()
            self.name = fam.name


_cases = {}


def case(fams, key):
    if key not in _cases:
        if key.startswith("deg_"):
            _cases[key] = Case(R.degenerate(key[4:]))
        elif key.endswith("_u16"):
            _cases[key] = Case(fams[key[:-4]], np.uint16)
        else:
            _cases[key] = Case(fams[key])
    return _cases[key]


DEPTH_KEYS = ["F1_clutter", "F2_ties", "F2_near_ties", "F2_ulp_ties", "F3_wide", "F3_97x61", "F3_300x200", "F4_near", "F4_far", "F5_mismatch", "F6_accept"]
ALL_KEYS = DEPTH_KEYS + [k + "_u16" for k in U16_TWINS] + ["deg_" + k for k in R.DEGENERATE]


def batch_of(clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate(clouds).astype(np.float32)), offs


def check_last_pass(rec_fitness, rec_rmse, cloud, oscene, ppb, where):
    """fitness / rmse of the product = those of the reference's canonical sums over the cloud as the product returned it."""
    s = O.sum29(cloud, oscene, O.SUM_CANONICAL, ppb)
    assert s[28] > 0, where
    assert np.float32(rec_fitness) == np.float32(s[28] / np.float32(len(cloud))), (where, rec_fitness, s[28])
    assert np.float32(rec_rmse) == np.float32(np.sqrt(np.float32(s[27] / s[28]))), (where, rec_rmse, s[27], s[28])


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_KEYS)
def test_every_pass_matches_the_reference_sums_of_the_returned_cloud(gpu, fams, key):
    """Bare ICP_Point2Plane and ICP_Point2Plane_batch, zero criteria, max_iteration = k for k in KS, host and device solve, default
    search options: the reported fitness and rmse equal float32(s[28] / n) and float32(sqrt(float32(s[27] / s[28]))) bit for bit,
    s = the oracle's canonical sums over the cloud the call returned (the positions of its last pass)."""
    c = case(fams, key)
    ppb = api.get_option("points_per_block")
    clouds = c.fam.clouds
    rng = np.random.default_rng(3)
    try:
        for solve in (api.SOLVE_HOST, api.SOLVE_DEVICE):
            api.set_option("solve", solve)
            for k in KS:
                crit = api.ICPConvergenceCriteria(0.0, 0.0, k)
                dev = api.DeviceVector.from_host(clouds[0].reshape(-1))
                r = api.ICP_Point2Plane(dev, c.scene, crit)
                got = dev.to_host().reshape(-1, 3)
                check_last_pass(r.fitness_, r.inlier_rmse_, got, c.oscene, ppb, (key, solve, k, "single"))
                q = got[rng.choice(len(got), min(32, len(got)), replace=False)]
                R.check_oracle_against_brute_force(c.oscene, q, R.BruteForce(q, c.oscene.pcd, c.fam.max_dist))
                flat, offs = batch_of(clouds)
                bdev = api.DeviceVector.from_host(flat.reshape(-1))
                recs = api.ICP_Point2Plane_batch(bdev, offs, c.scene, crit)
                bgot = bdev.to_host().reshape(-1, 3)
                for i in range(len(clouds)):
                    check_last_pass(recs["fitness"][i], recs["inlier_rmse"][i], bgot[offs[i]:offs[i + 1]], c.oscene, ppb, (key, solve, k, "batch", i))
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def _bare_runs(c, values):
    with options(**form(values)):
        dev = api.DeviceVector.from_host(c.fam.clouds[0].reshape(-1))
        r = api.ICP_Point2Plane(dev, c.scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
        flat, offs = batch_of(c.fam.clouds)
        bdev = api.DeviceVector.from_host(flat.reshape(-1))
        with options(solve=api.SOLVE_DEVICE):
            recs = api.ICP_Point2Plane_batch(bdev, offs, c.scene, api.ICPConvergenceCriteria())
        return (r.transformation_.tobytes(), r.fitness_, r.inlier_rmse_, dev.to_host().tobytes(), recs.tobytes(), bdev.to_host().tobytes())


@pytest.mark.parametrize("key", ALL_KEYS)
def test_search_forms_equal_the_stackless_walk_on_bare_calls(gpu, fams, key):
    """Bare single (fixed 20 passes, host solve) and batch (default criteria, device solve) calls: every search form returns the records
    and the clouds of the stackless walk, bit for bit."""
    c = case(fams, key)
    ref = _bare_runs(c, REF_FORM)
    assert ref[1] > 0.3
    for v in VARIANTS:
        assert _bare_runs(c, v) == ref, (key, v)


def _fused(fam, scene, values, crit, n_hyp=32):
    K = fam.K_fused if fam.K_fused is not None else fam.K
    proj = O.compute_proj(K, fam.W, fam.H)
    poses = synth.hypotheses(n_hyp)
    with options(**form(values)):
        res, sizes = api.refine_batch(fam.tris, poses, fam.W, fam.H, proj, K, scene, crit)
        api.refine_submit(0, fam.tris, poses[::-1], fam.W, fam.H, proj, K, scene, crit)
        ares, asizes = api.refine_wait(0)
    return res.tobytes(), sizes.tobytes(), ares.tobytes(), asizes.tobytes(), res, sizes


@pytest.mark.parametrize("key", ["F1_clutter", "F5_mismatch", "F1_clutter_u16"])
def test_search_forms_equal_the_stackless_walk_in_fused_batches(gpu, fams, key):
    """refine_batch of 32 hypotheses (fixed 20 passes and the default criteria) and a refine_submit / refine_wait pair: every search form
    gives the stackless walk's records bit for bit, and those equal the oracle's refine_batch in fitness.  F5: the hypotheses' camera is
    not the one the scene was made with (the pixel grid is built from projections under K')."""
    c = case(fams, key)
    fam = c.fam
    K = fam.K_fused if fam.K_fused is not None else fam.K
    ppb = api.get_option("points_per_block")
    for crit in ((0.0, 0.0, 20), (1e-5, 1e-5, 30)):
        ref = _fused(fam, c.scene, REF_FORM, api.ICPConvergenceCriteria(*crit))
        ores, osizes, _ = O.refine_batch(fam.tris, synth.hypotheses(32), fam.W, fam.H, O.compute_proj(K, fam.W, fam.H), K, c.oscene, crit,
                                         O.SUM_CANONICAL, ppb)
        assert np.array_equal(ref[5], osizes) and np.array_equal(ref[4]["fitness"], ores["fitness"]), (key, crit)
        assert ref[4]["fitness"].max() > 0.3
        for v in VARIANTS:
            got = _fused(fam, c.scene, v, api.ICPConvergenceCriteria(*crit))
            assert got[:4] == ref[:4], (key, crit, v)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
COUNT_PASSES = 31
_counts = {}


def _counted(c):
    """Bare ICP of the first cloud, 30 passes, default options, with and without counting: the same records; per-pass counters."""
    crit = api.ICPConvergenceCriteria(0.0, 0.0, COUNT_PASSES - 1)
    runs = []
    api.nn_counters(64)                                               # (reading resets them)
    for count in (0, 1):
        with options(nn_count=count):
            dev = api.DeviceVector.from_host(c.fam.clouds[0].reshape(-1))
            r = api.ICP_Point2Plane(dev, c.scene, crit)
            runs.append((r.transformation_.tobytes(), r.fitness_, r.inlier_rmse_, dev.to_host().tobytes()))
    cnt = api.nn_counters(COUNT_PASSES).astype(np.int64)
    assert runs[0] == runs[1]
    return cnt


@pytest.mark.parametrize("key", DEPTH_KEYS + ["deg_" + k for k in R.DEGENERATE])
def test_path_counters(gpu, fams, key):
    """Counting does not change the result.  Every query of a pass is kept (no search), settled by the window, or handed to the tree:
    queries >= window + tree in every pass (nn_search_kernel queues what it does not keep; nn_bound_kernel settles a queued query in the
    window or appends it to queue 2, from its main loop or from the deferred descent)."""
    c = case(fams, key)
    cnt = _counted(c)
    q, win, tree = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    assert np.all(q == len(c.fam.clouds[0])), q
    assert np.all(win + tree <= q) and win[0] + tree[0] == q[0]       # pass 0 has no previous winners: nothing is kept
    kept = q - win - tree
    _counts[key] = (int(q.sum()), int(win.sum()), int(tree.sum()), int(kept.sum()))
    print(f"\n{key}: queries {q.sum()}, window {win.sum()}, tree {tree.sum()}, kept {kept.sum()}, per pass window {win.tolist()}, tree {tree.tolist()}")
    if c.fam.depth is None:
        assert win.sum() == 0                                         # no camera: no pixel grid
    if key == "F2_ties":
        # pass 0: every query of the cloud is an exact tie between mirror-image points, which the window must refuse
        bf = R.BruteForce(c.fam.clouds[0], c.oscene.pcd, c.fam.max_dist)
        assert np.all(bf.n_ties() > 1)
        assert win[0] == 0 and tree[0] == q[0]


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("key", ["F3_97x61", "deg_coplanar"])
def test_all_eight_counter_columns(gpu, fams, key, wide):
    """Every column of api.nn_counters (enum NNCounter, nn_search.hip), per pass, on the two smallest inputs that reach every flush: F3_97x61
    (more than one search workgroup, several chunks per bound workgroup, a deferred list that is flushed in mid-loop) and deg_coplanar (no
    camera: the descent-to-leaf branch of nn_bound_kernel).  wide = 0 runs nn_tree_kernel instead of nn_bound_kernel + nn_tree_wide_kernel;
    a leaf holds at most 15 points in the wide records, max_leaf in the binary tree."""
    c = case(fams, key)
    with options(nn_wide=wide):
        cnt = _counted(c)
    q, win, tree, desc, nodes, leaves, leaf_pts, cells = (cnt[:, i] for i in range(8))
    print(f"\n{key} nn_wide={wide}:\n{cnt.tolist()}")
    per_leaf = 15 if wide else c.fam.max_leaf
    assert np.all(q == len(c.fam.clouds[0])), q
    assert np.all(win + tree <= q) and win[0] + tree[0] == q[0]
    assert np.all(desc <= win + tree), (desc, win, tree)              # a descent belongs to a query that was not kept
    if key == "F3_97x61":
        assert desc[0] > 0
    if c.fam.depth is None:
        assert not win.any() and not desc.any() and not cells.any()
    assert np.all((cells > 0) | (win == 0)), (cells, win)             # a window that settled a query was scanned
    for p in range(COUNT_PASSES):
        if tree[p] == 0:
            assert nodes[p] == 0 and leaves[p] == 0 and leaf_pts[p] == 0, (p, cnt[p])
        else:
            assert nodes[p] > 0 and leaves[p] > 0 and leaves[p] <= leaf_pts[p] <= per_leaf * leaves[p], (p, cnt[p])


def test_window_tree_and_kept_paths_are_all_taken(gpu, fams):
    """Over F1, F2 and F3 (640 wide) each path is taken: the pixel window settles queries, queries go to the tree, and winners are kept
    without a search; F1 and F3 take all three on their own."""
    tot = np.zeros(3, np.int64)
    for key in ("F1_clutter", "F2_ties", "F3_wide"):
        if key not in _counts:
            cnt = _counted(case(fams, key))
            q, win, tree = cnt[:, 0].sum(), cnt[:, 1].sum(), cnt[:, 2].sum()
            _counts[key] = (int(q), int(win), int(tree), int(q - win - tree))
        _, win, tree, kept = _counts[key]
        print(f"{key}: window {win} tree {tree} kept {kept}")
        if key != "F2_ties":
            assert win > 0 and tree > 0 and kept > 0, key
        tot += (win, tree, kept)
    assert np.all(tot > 0), tot
