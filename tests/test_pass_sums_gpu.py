"""GPU tests (-m gpu): the 29 sums of EVERY correspondence pass, as the product path delivered them, against the CPU oracle's canonical tree --
bit for bit, no tolerance anywhere.  pr_debug_trace_sums (api.trace_sums) records the rows the host-solve loop consumes; the oracle's
O.icp(..., SUM_CANONICAL, ppb, trace=True) says what they must be.  The inputs are windows of the scenario cloud that keep inliers at every size
(test_pass_sums_host.py holds that, and that another summation order would show): one point, partial wavefronts, sizes around 64 / 256 / 1024 /
points_per_block, 16 and 17 workgroups per cloud, clouds that start at odd point indices, every route the sums take to the host, the kd-tree
pass variants, the fused path's packed scene record, the device solve's score-only last pass and a grid smaller than the cloud needs.

Every traced test checks, as far as it applies: rows that must not be written are still NaN (an empty cloud, the passes after a hypothesis has
finished, one whole spare pass), a sentinel block behind the array is untouched, the number of written passes is the oracle's, and the records
of the traced call equal those of the same call untraced, byte for byte."""
import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import *  # noqa: F401,F403 -- W, H, TOL_T, inliers ...
from pass_sums_ref import NN_SIZES, PPBS, differing_columns, expect_rows, odd_start_order, oracle_trace, sizes_for, u32, window

pytestmark = pytest.mark.gpu

SENTINEL_WORDS, SENTINEL = 1024, 0xA5C3F00D
CRIT_PROJ, CRIT_NN = (0.0, 0.0, 3), (0.0, 0.0, 2)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def traced(n_hyp, n_passes, call):
    """Runs call() with the recorder armed on an array that has a sentinel block behind it; returns (call's result, (n_passes, n_hyp, 29) rows)."""
    n = n_passes * n_hyp * 29
    buf = np.full(n + SENTINEL_WORDS, np.nan, np.float32)
    tail = buf[n:].view(np.uint32)
    tail[:] = SENTINEL
    lib = _lib.load()
    _lib.check(lib.pr_debug_trace_sums(buf.ctypes.data, n_hyp, n_passes))
    try:
        out = call()
    finally:
        _lib.check(lib.pr_debug_trace_sums(None, 0, 0))
    assert (tail == SENTINEL).all(), "the recorder wrote behind its array"
    return out, buf[:n].reshape(n_passes, n_hyp, 29)


def ragged(clouds):
    offs = np.cumsum([0] + [len(c) for c in clouds]).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate(clouds), np.float32), offs


def icp_batch(flat, offs, scene, crit):
    return api.ICP_Point2Plane_batch(api.DeviceVector.from_host(flat.reshape(-1)), offs, scene, api.ICPConvergenceCriteria(*crit))


def written_passes(rows):
    """Per hypothesis: how many leading passes carry a row (and nothing after them does)."""
    have = ~np.isnan(rows).all(axis=2)                             # (n_passes, n_hyp)
    count = have.sum(axis=0)
    for i, c in enumerate(count):
        assert have[:c, i].all() and not have[c:, i].any(), (i, have[:, i])
    return count


def solve_attribution(clouds, scene, crit, ppb, i, it):
    """For a small (rank-deficient) cloud whose pass `it` differs while pass it-1 agrees: does the host-solve loop's iteration on the ORACLE's
    row of pass it-1 give the oracle's update?  (text for the failure message; the comparison itself is never relaxed)"""
    _, _, tr = oracle_trace(clouds[i], scene, crit, ppb)
    s = tr[it - 1]
    A = np.zeros((6, 6), np.float32)
    k = 0
    for y in range(6):
        for x in range(y, 6):
            A[y, x] = A[x, y] = s[k]; k += 1
    want = O.solve666(A, s[21:27])
    _, upd, _ = api.debug_pose_iteration(s[None], [len(clouds[i])], api.ICPConvergenceCriteria(*crit), it - 1, on_device=False)
    same = np.array_equal(u32(upd[0]), u32(want))
    return f"host iteration on the oracle's row of pass {it - 1} {'equals' if same else 'DIFFERS from'} O.solve666 (max |d| {np.abs(upd[0] - want).max():.3g})"


def assert_rows(rows, clouds, scene, crit, ppb, what):
    """rows == the oracle's traces, as uint32; on a mismatch the message names pass, cloud size and the number of differing columns, pass 0 first."""
    want, recs, passes = expect_rows(rows.shape[0], clouds, scene, crit, ppb)
    got_passes = written_passes(rows)
    bad = []
    for i, cl in enumerate(clouds):
        if len(cl) == 0:
            assert np.isnan(rows[:, i]).all(), (what, i, "an empty cloud got a row")
            continue
        for it in range(rows.shape[0]):
            d = differing_columns(rows[it, i], want[it, i])
            if d:
                bad.append((it, i, len(cl), d))
    if bad:
        bad.sort()
        it, i, n, _ = bad[0]
        note = ""
        if it > 0 and n < 63 and not any(b[1] == i and b[0] < it for b in bad):
            note = " -- " + solve_attribution(clouds, scene, crit, ppb, i, it)
        pytest.fail(f"{what}: {len(bad)} rows differ from the canonical tree; (pass, cloud, points, differing columns) = {bad[:12]}{note}")
    assert np.array_equal(got_passes, passes), (what, got_passes, passes)
    assert np.array_equal(u32(rows), u32(want)), what              # (the whole array at once: NaN rows included)
    return recs, passes


def assert_records(res, recs, clouds, what):
    """The records of a host-solve call against the oracle's: scores exact (functions of sums 27 and 28), transforms within the suite's 1e-4.
    T is not compared here for clouds under 63 points (a rank-deficient system): the rows of their later passes, which assert_rows holds bit for
    bit, are sums over the cloud moved by those transforms, so a transform that differed would show there."""
    for i, (cl, o) in enumerate(zip(clouds, recs)):
        if o is None:
            assert res[i]["fitness"] == 0.0 and res[i]["inlier_rmse"] == 0.0 and np.array_equal(res[i]["T"], np.eye(4, dtype=np.float32).reshape(-1)), (what, i)
            continue
        assert res[i]["fitness"] == o["fitness"] and res[i]["inlier_rmse"] == o["inlier_rmse"], (what, i, len(cl))
        if len(cl) >= 63:
            assert np.allclose(res[i]["T"], o["T"], rtol=0, atol=TOL_T), (what, i, len(cl))


def proj_parts(cloud, ppb):
    """The ragged batch of (a): every size of this points_per_block and an empty cloud, ordered for odd starts, then the full cloud."""
    order = odd_start_order(sizes_for(ppb, len(cloud)) + [0])
    return [window(cloud, n) for n in order] + [cloud]


class options:
    """with options(name=value, ...): set, and restore what was there."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: api.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            api.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            api.set_option(k, v)


# ---- a. projective scene, pr_icp_batch, ragged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppb", PPBS)
def test_projective_ragged_batch_every_pass(gpu, scenario, gscenes, ppb):
    """icp_pass_kernel<SceneProjAoS> with fused = 2 (sums finalized in the pass tail, stored into pinned memory): four passes, three of them with the
    pending transform, at 1024 (16 / 17 workgroups cross sum_partials' chunk), 3072 and 65 536 points per workgroup (the cloud is one block)."""
    cloud = scenario["cloud"]
    parts = proj_parts(cloud, ppb)
    flat, offs = ragged(parts)
    assert (offs[:-1] % 2 == 1).sum() > len(parts) // 2
    with options(points_per_block=ppb):
        res, rows = traced(len(parts), CRIT_PROJ[2] + 2, lambda: icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ))
        plain = icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)
        recs, passes = assert_rows(rows, parts, scenario["proj_scene"], CRIT_PROJ, ppb, f"ppb {ppb}")
        assert res.tobytes() == plain.tobytes()
        assert_records(res, recs, parts, f"ppb {ppb}")
        assert max(passes) == CRIT_PROJ[2] + 1


@pytest.mark.parametrize("n", [65, 3073])
def test_projective_single_cloud_every_pass(gpu, scenario, gscenes, n):
    """pr_icp_proj (a batch of one: cloud start 0), through api.trace_sums."""
    cl = window(scenario["cloud"], n)
    crit = api.ICPConvergenceCriteria(*CRIT_PROJ)
    rows = api.trace_sums(1, CRIT_PROJ[2] + 1)
    r = api.ICP_Point2Plane(api.DeviceVector.from_host(cl.reshape(-1)), gscenes["proj"], crit)
    plain = api.ICP_Point2Plane(api.DeviceVector.from_host(cl.reshape(-1)), gscenes["proj"], crit)      # the recorder is gone: `rows` stays as it is
    recs, _ = assert_rows(rows, [cl], scenario["proj_scene"], CRIT_PROJ, api.get_option("points_per_block"), f"single {n}")
    assert r.fitness_ == plain.fitness_ == recs[0]["fitness"] and r.inlier_rmse_ == plain.inlier_rmse_ == recs[0]["inlier_rmse"]
    assert np.array_equal(r.transformation_, plain.transformation_)


# ---- b. the routes may not change a bit ---------------------------------------------------------------------------------------------------
def test_routes_to_the_host_do_not_change_a_bit(gpu, scenario, gscenes):
    """130 clouds (4 real pose groups): sums stored by the pass tail into pinned memory or finalized by a launch of their own and copied
    (fused_solve 1 / 0), the host polling flags or waiting for the stream (host_poll), one or four pose groups -- one trace, the oracle's."""
    cloud = scenario["cloud"]
    ppb = api.get_option("points_per_block")
    order = odd_start_order(sizes_for(ppb, len(cloud)) + [0])
    parts = [window(cloud, n) for n in (order * 6)[:130]]
    flat, offs = ragged(parts)
    plain = icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)
    first = None
    for fused in (1, 0):
        for poll in (1, 0):
            for groups in (1, 4):
                what = f"fused_solve {fused} host_poll {poll} pose_groups {groups}"
                with options(fused_solve=fused, host_poll=poll, pose_groups=groups):
                    res, rows = traced(len(parts), CRIT_PROJ[2] + 2, lambda: icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ))
                if first is None:
                    assert_rows(rows, parts, scenario["proj_scene"], CRIT_PROJ, ppb, what)
                    first = rows
                assert rows.tobytes() == first.tobytes(), what
                assert res.tobytes() == plain.tobytes(), what
    assert api.get_option("stat_flag_overtook") == 0


# ---- c. kd-tree scene --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(nn_split=1), dict(nn_split=0, nn_stack=1, nn_compact=1), dict(nn_split=0, nn_stack=1, nn_compact=0),
                                 dict(nn_split=0, nn_stack=0)], ids=["search+winners", "fused-stack-compact", "fused-stack-exact", "fused-stackless"])
def test_kdtree_pass_variants_every_pass(gpu, scenario, gscenes, cfg):
    """The winners pass behind the search kernel (kStack = -1), the search fused into the pass with the per-lane stack on compact and on exact
    records, and the stackless walk: each delivers the oracle's kd-tree sums in the canonical tree.  (A differing row is first a question for
    api.debug_contrib29 -- did a WINNER differ?  That is the search, which test_nn_exact_gpu.py holds -- and only then one for the tree.)"""
    cloud = scenario["cloud"]
    parts = [window(cloud, n) for n in odd_start_order(list(NN_SIZES) + [0])]
    flat, offs = ragged(parts)
    ppb = api.get_option("points_per_block")
    plain = icp_batch(flat, offs, gscenes["nn"], CRIT_NN)          # (default options)
    with options(**cfg):
        res, rows = traced(len(parts), CRIT_NN[2] + 2, lambda: icp_batch(flat, offs, gscenes["nn"], CRIT_NN))
    recs, passes = assert_rows(rows, parts, scenario["nn_scene"], CRIT_NN, ppb, str(cfg))
    assert res.tobytes() == plain.tobytes()
    assert_records(res, recs, parts, str(cfg))
    assert max(passes) == CRIT_NN[2] + 1


# ---- d. fused path, packed scene record -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi", [None, (160, 80, 320, 240)], ids=["full-frame", "roi"])
def test_fused_batch_every_pass(gpu, model, scenario, gscenes, roi):
    """pr_refine_batch[_roi] under host solve: icp_pass_kernel<SceneProjPacked> on the rendered clouds, packed one behind the other at
    kCloudAlign-rounded starts.  Row (it, i) is the oracle's trace on the oracle's own render of hypothesis i."""
    poses = synth.hypotheses(6)
    poses[2] = poses[2].copy(); poses[2][0, 3] += 1.0e6                                    # off screen: an empty cloud
    K, proj = scenario["K"], scenario["proj"]
    crit = api.ICPConvergenceCriteria(*CRIT_PROJ)
    oroi = roi or (0, 0, 0, 0)
    clouds = [O.depth2cloud(O.render(scenario["tris"], poses[i:i + 1], W, H, proj, oroi)[0], K, 1, oroi[0], oroi[1]) for i in range(len(poses))]
    assert len(clouds[2]) == 0 and min(len(c) for i, c in enumerate(clouds) if i != 2) > 3072
    (res, sizes), rows = traced(len(poses), CRIT_PROJ[2] + 2, lambda: api.refine_batch(model, poses, W, H, proj, K, gscenes["proj"], crit, roi=roi))
    plain, psizes = api.refine_batch(model, poses, W, H, proj, K, gscenes["proj"], crit, roi=roi)
    assert np.array_equal(sizes, [len(c) for c in clouds]) and np.array_equal(sizes, psizes)
    recs, _ = assert_rows(rows, clouds, scenario["proj_scene"], CRIT_PROJ, api.get_option("points_per_block"), f"refine_batch roi {roi}")
    assert res.tobytes() == plain.tobytes()
    assert_records(res, recs, clouds, f"refine_batch roi {roi}")


# ---- e. device solve: the score-only last pass ------------------------------------------------------------------------------------------------
@pytest.mark.device_solve
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_device_solve_last_pass_scores(gpu, scenario, gscenes, k):
    """Under device solve the last pass reduces sums 27 and 28 alone (vb_reduce<true>) and nothing is traced: fitness and rmse of every cloud are
    exact functions of the oracle's row k.  Pass 0 depends on no solve and holds for every size; later passes for the sizes whose 6x6 system has
    full rank (>= 63 points) -- a difference there is the device solve disagreeing with the host solve, a finding for test_solve_gpu's corpus.
    Sum 28 is a count, exact in any order: only sum 27 can show a wrong tree here, and on one pass it does so for few clouds (restating the
    wave tree with two levels swapped changes sum 27 of no cloud of this batch at pass 0, of one each at passes 1 and 2, of two at pass 3) --
    hence every last pass from 0 to 3, not 0 and 2 alone."""
    cloud = scenario["cloud"]
    ppb = api.get_option("points_per_block")
    parts = proj_parts(cloud, ppb)
    flat, offs = ragged(parts)
    crit = (0.0, 0.0, k)
    got = {}
    for fused in (1, 0):
        for graph in (1, 0):
            with options(fused_solve=fused, graph=graph):
                got[fused, graph] = icp_batch(flat, offs, gscenes["proj"], crit)
    for (fused, graph), res in got.items():
        for i, cl in enumerate(parts):
            what = (k, fused, graph, i, len(cl))
            if len(cl) == 0:
                assert res[i]["fitness"] == 0.0 and res[i]["inlier_rmse"] == 0.0, what
                continue
            if k > 0 and len(cl) < 63:
                continue
            rec, passes, tr = oracle_trace(cl, scenario["proj_scene"], crit, ppb)
            assert passes == k + 1 and tr[k][28] > 0, what
            s = tr[k]
            assert res[i]["fitness"] == np.float32(s[28] / np.float32(len(cl))), what
            assert res[i]["inlier_rmse"] == np.float32(np.sqrt(np.float32(s[27] / s[28]))), what
            assert np.allclose(res[i]["T"], rec["T"], rtol=0, atol=TOL_T), what


# ---- f. a grid smaller than the cloud needs -----------------------------------------------------------------------------------------------------
@pytest.mark.device_solve
def test_grid_smaller_than_the_cloud_needs(gpu, model, scenario, gscenes):
    """The asynchronous path sizes a batch's grid by the largest cloud of the batch BEFORE it on the context: after a batch of far-away
    hypotheses (small clouds) the workgroups of a batch of near ones loop over virtual blocks (vb += gridDim.x).  Here by construction, at 1024
    points per workgroup: 3 workgroups walk 26 blocks.  Records and sizes equal the same batch on a full grid, byte for byte."""
    K, proj = scenario["K"], scenario["proj"]
    crit = api.ICPConvergenceCriteria(*CRIT_PROJ)
    near = synth.hypotheses(8)
    far = near.copy()
    far[:, 2, 3] *= 3.0                                            # three times as far: a ninth of the pixels
    with options(points_per_block=1024):
        api.refine_submit(0, model, far, W, H, proj, K, gscenes["proj"], crit)
        _, far_sizes = api.refine_wait(0)
        api.refine_submit(0, model, near, W, H, proj, K, gscenes["proj"], crit)
        res, sizes = api.refine_wait(0)
        blocks = lambda s: (int(max(s)) + 1023) // 1024
        assert 0 < blocks(far_sizes) < blocks(sizes), (far_sizes, sizes)        # grid_x < used
        full, fsizes = api.refine_batch(model, near, W, H, proj, K, gscenes["proj"], crit)   # (its grid comes from the near batch before it)
        assert np.array_equal(sizes, fsizes) and res.tobytes() == full.tobytes()
        ores, osizes, _ = O.refine_batch(scenario["tris"], near, W, H, proj, K, scenario["proj_scene"], CRIT_PROJ, O.SUM_CANONICAL, 1024)
        assert np.array_equal(sizes, osizes) and np.array_equal(res["fitness"], ores["fitness"])
        assert np.allclose(res["T"], ores["T"], rtol=0, atol=TOL_T)


# ---- g. contract ------------------------------------------------------------------------------------------------------------------------
def test_recorder_contract(gpu, scenario, gscenes):
    """The traced call is refused (PR_ERR_INVALID, nothing written) under device solve, for another batch size and for too few passes; a refusal
    disarms the recorder, and the next call -- untraced -- gives the usual bytes."""
    cloud = scenario["cloud"]
    parts = [window(cloud, 65), window(cloud, 257)]
    flat, offs = ragged(parts)
    plain = icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)

    def refused(n_hyp, n_passes, **opts):
        with options(**opts):
            rows = api.trace_sums(n_hyp, n_passes)
            with pytest.raises(api.PoseRefineError) as e:
                icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)
            assert e.value.code == _lib.PR_ERR_INVALID and "pr_debug_trace_sums" in str(e.value)
            after = icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)       # the recorder is gone: this call runs, and leaves `rows` alone
        assert np.isnan(rows).all()
        return after

    assert refused(2, 4, solve=api.SOLVE_DEVICE).tobytes() == icp_batch_device(flat, offs, gscenes["proj"]).tobytes()
    assert refused(3, 4).tobytes() == plain.tobytes()
    assert refused(1, 4).tobytes() == plain.tobytes()
    assert refused(2, 3).tobytes() == plain.tobytes()
    # a list that runs in pieces (more than 32 768 clouds) is refused as a whole: rows are indexed within one run
    many = np.minimum(np.arange(32770), 65).astype(np.uint32)      # offsets of 32 769 clouds: 65 one-point clouds, then empty ones
    rows = api.trace_sums(32769, 1)
    with pytest.raises(api.PoseRefineError) as e:
        icp_batch(flat, many, gscenes["proj"], (0.0, 0.0, 0))
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_debug_trace_sums" in str(e.value) and np.isnan(rows).all()
    assert icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ).tobytes() == plain.tobytes()
    # armed, then disarmed by hand: nothing is recorded
    rows = api.trace_sums(2, 4)
    api.trace_sums_off()
    assert icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ).tobytes() == plain.tobytes() and np.isnan(rows).all()
    # one call per arming: the second call of a pair is not recorded
    rows = api.trace_sums(2, 4)
    icp_batch(flat, offs, gscenes["proj"], CRIT_PROJ)
    seen = rows.copy()
    assert not np.isnan(seen).any()
    icp_batch(flat[::-1].copy(), offs, gscenes["proj"], CRIT_PROJ)
    assert rows.tobytes() == seen.tobytes()


def icp_batch_device(flat, offs, scene):
    with options(solve=api.SOLVE_DEVICE):
        return icp_batch(flat, offs, scene, CRIT_PROJ)
