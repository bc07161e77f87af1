"""GPU tests (-m gpu) of the two kd-tree walks inside icp_pass_kernel at every size of their LDS staging: the stackless walk (option
nn_lds_nodes: leading 16-byte topology entries, up to 8192 = 128 KiB, beyond 64 KiB by a per-device opt-in) and the per-lane-stack walk on exact
64-byte records (option nn_lds_records: up to 504 records beside 16-entry stacks, 248 beside 24-entry ones), the robust instantiation of the
former, the default route of a tree deeper than any stack (nn_ref.vine), and option nn_run of the split route.

References, none of them the code under test:
(r1) the oracle's canonical sums of every pass, bit for bit (assert_rows / assert_records of test_pass_sums_gpu.py on the family's O.NNScene);
(r2) brute force: the first pass's inlier count (sum 28 of pass 0) is the number of queries with a scene point inside the acceptance radius
     in the reference's float32 arithmetic (nn_ref.inside_count, held to nn_ref.BruteForce in test_nn_ref.py);
(r3) byte identity of the result records and the returned cloud across all settings of a route on a scene, and with the library defaults.
The read-only options stat_nn_lds_nodes / stat_nn_stack_depth say what the most recent in-pass launch really staged and which walk it took,
and stat_nn_pass_launches counts those launches (one per pass of a host-solve call), so a setting that quietly ran unstaged, or on another
route -- leaving the two values of the call before it -- fails here.

Not run: a fused refine_batch on the vine -- the vine is a hand-made point set without a depth image or camera, and a mesh whose renders
land on it would be a second construction; the bare calls run the same kernel instantiation.
"""
import numpy as np
import pytest

import nn_ref as R
import oracle_lib as O
import robust_ref
from gpu_common import make_scene
from pose_refine_amd import _lib, api
from test_nn_exact_gpu import Case
from test_pass_sums_gpu import assert_records, assert_rows, options, traced

pytestmark = pytest.mark.gpu

CRIT = (0.0, 0.0, 3)                                              # four passes, three of them with a pending transform
STACKLESS = dict(nn_split=0, nn_stack=0)
STACK_EXACT = dict(nn_split=0, nn_stack=1, nn_compact=0)
NODES_MAX = 8192                                                  # nn_lds_nodes beyond it stages 8192 (128 KiB)
RECORDS_MAX = {16: 504, 24: 248}                                  # 64 KiB - 512 static bytes - stacks, in 64-byte records
DEFAULT_NODES = 1024


class Sc:
    """A scene of the product with the oracle's twin, the cloud the tests query it with, and what the runs share."""

    def __init__(self, name, scene, oscene, cloud, max_dist):
        self.name, self.scene, self.oscene, self.max_dist = name, scene, oscene, max_dist
        self.cloud = np.ascontiguousarray(cloud, np.float32)
        self.n_nodes = len(oscene.nodes)
        self.default = None                                          # (records, cloud) bytes at the library defaults


def scene_of_tree(pts, nrm, nodes, max_dist):
    """A Scene_nn over a tree the caller made (the vine): the three arrays uploaded as they are."""
    s = api.Scene_nn()
    s.max_dist_diff = max_dist
    s.pcd_host, s.normal_host = pts, nrm
    s.nodes_host = np.ascontiguousarray(nodes).view(_lib.KDNODE)
    s.pcd_buffer = api.DeviceVector.from_host(pts.reshape(-1))
    s.normal_buffer = api.DeviceVector.from_host(nrm.reshape(-1))
    s.nodes = api.DeviceVector.from_host(s.nodes_host)
    return s


_scenes = {}


def sc_of(key):
    if key in _scenes:
        return _scenes[key]
    if key == "vine":
        fam = R.vine()
        s = Sc(key, scene_of_tree(fam.pts, fam.nrm, fam.nodes, fam.max_dist), fam.oracle_scene(), fam.clouds[0], fam.max_dist)
        assert R.tree_depth(fam.nodes) > 24
    elif key == "deep":                                               # the tree of test_deep_tree_runs_the_24_entry_stacks_in_every_search_form
        rng = np.random.default_rng(77)
        pts = rng.uniform(-0.2, 0.2, size=(140000, 3)).astype(np.float32)
        nrm = rng.normal(size=(140000, 3)).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        scene = make_scene(pts, nrm, 1, max_dist=0.02)                # (reorders pts / nrm in place)
        assert 16 < R.tree_depth(scene.nodes_host) <= 24
        cloud = rng.uniform(-0.2, 0.2, size=(3000, 3)).astype(np.float32)
        s = Sc(key, scene, O.NNScene.from_points(pts, nrm, 0.02, nodes=scene.nodes_host), cloud, 0.02)
    else:
        fam = R.degenerate(key[4:]) if key.startswith("deg_") else {"F3_97x61": lambda: R.f3_small(97, 61), "F3_300x200": lambda: R.f3_small(300, 200)}[key]()
        c = Case(fam)
        s = Sc(key, c.scene, c.oscene, fam.clouds[0], fam.max_dist)
    assert 2000 <= len(s.cloud) <= 19007
    _scenes[key] = s
    return s


def stat():
    return api.get_option("stat_nn_lds_nodes"), api.get_option("stat_nn_stack_depth")


def run(s, opts, trace=False, robust=None, crit=CRIT, in_pass=True):
    """One bare batch call of the scene's cloud under `opts`.  Returns ((records, cloud) bytes, what the in-pass launch ran with, records, rows).
    in_pass: the call must have searched inside the pass, one launch per pass (True), or not at all (False: the split route); None: not checked
    (a replayed graph enqueues nothing)."""
    offs = np.array([0, len(s.cloud)], np.uint32)
    dev = api.DeviceVector.from_host(s.cloud.reshape(-1))
    call = lambda: api.ICP_Point2Plane_batch(dev, offs, s.scene, api.ICPConvergenceCriteria(*crit), robust=robust)
    with options(**opts):
        before = api.get_option("stat_nn_pass_launches")
        res, rows = traced(1, crit[2] + 2, call) if trace else (call(), None)
        ran = stat()
        launches = (api.get_option("stat_nn_pass_launches") - before) % 2**31
    if in_pass is not None:
        assert launches == (crit[2] + 1 if in_pass else 0), (s.name, opts, launches)
    return (res.tobytes(), dev.to_host().tobytes()), ran, res, rows


def defaults(s):
    if s.default is None:
        s.default = run(s, {}, in_pass=True if s.name == "vine" else None)[0]     # (whatever route the scene takes; the vine must search in the pass)
    return s.default


def hold_r1(s, res, rows, what):
    ppb = api.get_option("points_per_block")
    recs, passes = assert_rows(rows, [s.cloud], s.oscene, CRIT, ppb, what)
    assert_records(res, recs, [s.cloud], what)
    assert max(passes) == CRIT[2] + 1, what
    return rows


def hold_r2(s, rows, what):
    want = R.inside_count(s.cloud, s.oscene.pcd, s.max_dist)
    print(f"{what}: first-pass inliers {int(rows[0, 0, 28])} of {len(s.cloud)}, brute force {want}")
    assert 0 < want and float(rows[0, 0, 28]) == float(want), what


# ---- the stackless walk ------------------------------------------------------------------------------------------------------------------
STACKLESS_CASES = {"F3_300x200": (16245, (0, 1, 1023, 1024, 4096, 4097, 8191, 8192, 20000)),
                   "F3_97x61": (1569, (0, 1, 1568, 1569, 1570, 8192)),
                   "deg_repeated": (127, (0, 126, 127, 1024))}


@pytest.mark.parametrize("key", list(STACKLESS_CASES))
def test_stackless_walk_at_every_staging_size(gpu, key):
    """nn_split = 0, nn_stack = 0: no staging at all, one entry, both sides of lds_nodes around the default / the 64 KiB line / the tree's last node /
    the 8192 cap, the whole tree, a request beyond the tree.  Every setting stages min(setting, tree, 8192) entries on the stackless walk
    (8192 on the largest tree: the opt-in beyond 64 KiB is granted) and returns the bytes of the library defaults; the sums of every pass are the
    oracle's at 0, at the default and at the largest setting; the first pass's inlier count is brute force's."""
    n_nodes, settings = STACKLESS_CASES[key]
    s = sc_of(key)
    assert s.n_nodes == n_nodes
    want = defaults(s)
    r1_at = {0, DEFAULT_NODES, max(settings)}
    first_rows = None
    for v in sorted(set(settings) | r1_at):
        what = f"{key} stackless nn_lds_nodes {v}"
        got, ran, res, rows = run(s, dict(STACKLESS, nn_lds_nodes=v), trace=v in r1_at)
        print(f"{what}: ran {ran}")
        assert ran == (min(v, n_nodes, NODES_MAX), 0), what
        assert got == want, what
        if v in r1_at:
            hold_r1(s, res, rows, what)
            first_rows = rows if first_rows is None else first_rows
    hold_r2(s, first_rows, key)


def test_vine_takes_the_stackless_walk_by_itself(gpu):
    """A tree 63 levels deep at the library defaults: nn_route itself picks the stackless walk (no nn_stack = 0 here) and stages the whole tree,
    127 entries; with nn_lds_nodes 0, 1 and 63 the walk crosses from LDS to memory at the root, below it and half way down.  The oracle's sums
    in every pass at every setting, brute force's first-pass count, one set of bytes."""
    s = sc_of("vine")
    assert s.n_nodes == 127
    got0, ran, res, rows = run(s, {}, trace=True)
    assert ran == (127, 0)
    hold_r1(s, res, rows, "vine defaults")
    hold_r2(s, rows, "vine")
    assert got0 == defaults(s)
    for v in (0, 1, 63):
        got, ran, res, rows = run(s, dict(nn_lds_nodes=v), trace=True)
        assert ran == (v, 0), v
        assert got == got0, v
        hold_r1(s, res, rows, f"vine nn_lds_nodes {v}")
    assert run(s, STACKLESS)[0] == got0


# ---- the per-lane-stack walk on exact records --------------------------------------------------------------------------------------------------
# (the issue's settings around 512 / 256, and both sides of the caps as they are now: 504 / 248)
STACK_CASES = {"F3_97x61": (16, (0, 1, 64, 503, 504, 505, 511, 512, 513)),
               "deg_repeated": (16, (0, 127, 512)),
               "deep": (24, (0, 247, 248, 249, 255, 256, 257))}


@pytest.mark.parametrize("key", list(STACK_CASES))
def test_exact_record_stack_walk_at_every_staging_size(gpu, key):
    """nn_split = 0, nn_stack = 1, nn_compact = 0: the staging loop behind the stacks and the LDS branch of query_nn_stack_from.  Every setting
    stages min(setting, tree, cap) records beside 16- or 24-entry stacks and returns the bytes of the stackless walk and of the library
    defaults; the oracle's sums in every pass without staging and at the cap."""
    depth, settings = STACK_CASES[key]
    s = sc_of(key)
    assert (R.tree_depth(s.oscene.nodes) <= 16) == (depth == 16) and R.tree_depth(s.oscene.nodes) <= 24
    cap = min(s.n_nodes, RECORDS_MAX[depth])
    want = defaults(s)
    stackless, ran, _, _ = run(s, STACKLESS)
    assert ran == (min(DEFAULT_NODES, s.n_nodes), 0) and stackless == want
    for v in settings:
        what = f"{key} stack-exact nn_lds_records {v}"
        trace = v in (0, max(settings))
        got, ran, res, rows = run(s, dict(STACK_EXACT, nn_lds_records=v), trace=trace)
        print(f"{what}: ran {ran}")
        assert ran == (min(v, cap), depth), what
        assert got == want, what
        if trace:
            hold_r1(s, res, rows, what)
    assert ran == (cap, depth)                                       # (the last setting asked for more than the cap)


# ---- the robust instantiation of the stackless walk -----------------------------------------------------------------------------------------------
def test_robust_stackless_walk_at_every_staging_size(gpu):
    """A robust call on a scene without compact records searches in the pass with the stackless walk's robust instantiation, beside whatever
    stack_depth the route carries: it stages nn_lds_nodes entries like the plain one.  One set of bytes, those of the default options (the
    split route, which test_robust_gpu.py holds to its reference)."""
    s = sc_of("F3_97x61")
    rb = api.Robust(robust_ref.HUBER, 0.005)
    want = run(s, {}, robust=rb, in_pass=False)[0]
    for v in (0, 1024, 1569, 8192):
        got, ran, _, _ = run(s, dict(nn_split=0, nn_compact=0, nn_lds_nodes=v), robust=rb)
        assert ran == (min(v, s.n_nodes), 0), v
        assert got == want, v
    assert want != defaults(s)                                       # (the weight does something on this cloud)


# ---- device solve: a replayed graph reports what it captured ------------------------------------------------------------------------------------
@pytest.mark.device_solve
def test_device_solve_reports_the_staging_of_a_replayed_graph(gpu):
    """Under device solve the loop of a bare call is captured once per setting and replayed afterwards: the stat options follow the graph that
    ran, not the launch that was enqueued last; the bytes do not depend on the setting."""
    s = sc_of("deg_repeated")
    first = None
    for v in (0, 127, 0, 64, 127):
        got, ran, _, _ = run(s, dict(STACKLESS, nn_lds_nodes=v), in_pass=None)
        assert ran == (v, 0), v
        first = first or got
        assert got == first, v
    got, ran, _, _ = run(s, dict(STACK_EXACT, nn_lds_records=32), in_pass=None)
    assert ran == (32, 16) and got == first


# ---- nn_run -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["F3_97x61", "F3_300x200"])
def test_nn_run_does_not_change_a_byte(gpu, key):
    """The split route at the library defaults with 1, 3, 8 and 9 (= 8) chunks of 256 points per search workgroup; 5598 and 19 007 points are
    no multiple of 256 * run for any of them.  The oracle's sums in every pass at 1; one set of bytes."""
    s = sc_of(key)
    assert all(len(s.cloud) % (256 * r) for r in (1, 3, 8))
    want = defaults(s)
    for v in (1, 3, 8, 9):
        with options(nn_run=v):
            assert api.get_option("nn_run") == min(v, 8)
            got, _, res, rows = run(s, {}, trace=v == 1, in_pass=False)
        assert got == want, v
        if v == 1:
            hold_r1(s, res, rows, f"{key} nn_run 1")


# ---- the options themselves ----------------------------------------------------------------------------------------------------------------------------
def test_option_read_back(gpu):
    """Negative staging requests read back 0, nn_run reads back what the search takes (1..8), the stat options refuse writes and the defaults
    are 1024 / 0 / 8."""
    assert (api.get_option("nn_lds_nodes"), api.get_option("nn_lds_records"), api.get_option("nn_run")) == (1024, 0, 8)
    for name, pairs in (("nn_lds_nodes", ((-1, 0), (-2**31, 0), (0, 0), (20000, 20000))), ("nn_lds_records", ((-7, 0), (513, 513))),
                        ("nn_run", ((-3, 1), (0, 1), (1, 1), (8, 8), (9, 8), (256, 8), (2**31 - 1, 8)))):
        for value, back in pairs:
            with options(**{name: value}):
                assert api.get_option(name) == back, (name, value)
    for name in ("stat_nn_lds_nodes", "stat_nn_stack_depth", "stat_nn_pass_launches"):
        before = api.get_option(name)
        with pytest.raises(api.PoseRefineError) as e:
            api.set_option(name, 5)
        assert e.value.code == _lib.PR_ERR_INVALID and api.get_option(name) == before
    assert (api.get_option("nn_lds_nodes"), api.get_option("nn_lds_records"), api.get_option("nn_run")) == (1024, 0, 8)
