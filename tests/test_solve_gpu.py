"""GPU tests (-m gpu): the device's wavefront iteration (pose_iteration_wave, what the fused pass tail and icp_finalize_solve_kernel
run) against the host-solve loop's iteration and the Python restatement, bit for bit, over the corpus of tests/solve_ref.py: all 720
pivot sequences, the branch edges of the solver, the iteration-logic edges and ICP-realistic systems (pr_debug_pose_iteration)."""
import numpy as np
import pytest

import solve_ref as R
from pose_refine_amd import api
from test_solve_ref import same_bits, spd_rows, state_of, truth_bound
from truth_ref import float64_truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches(gpu, scenario):
    return R.solve_batches(scenario) + R.iteration_batches()


def both_routes(b):
    crit = api.ICPConvergenceCriteria(*b.crit)
    dev = api.debug_pose_iteration(b.sums, b.n_points, crit, b.it, True, state_of(b))
    host = api.debug_pose_iteration(b.sums, b.n_points, crit, b.it, False, state_of(b))
    return dev, host


def test_device_iteration_equals_host_bitwise(batches):
    """E, the new T, fitness, rmse and the finished flag: device route == host route on every batch (NaN compared by mask;
    denormal inputs get no special case)."""
    for b in batches:
        (sd, Ed, fd), (sh, Eh, fh) = both_routes(b)
        bad = [i for i in range(len(b.sums))
               if not (fd[i] == fh[i] and same_bits(Ed[i], Eh[i]) and same_bits(sd["T"][i], sh["T"][i])
                       and same_bits(sd["fitness"][i], sh["fitness"][i]) and same_bits(sd["inlier_rmse"][i], sh["inlier_rmse"][i]))]
        assert not bad, (b.name, [(i, b.tags[i]) for i in bad[:10]])


def test_device_updates_equal_restatement(batches):
    """The device's E equals the Python restatement of prs::solve_666_impl on the whole solve corpus, and every pivot sequence ran."""
    b = batches[0]
    (sd, Ed, fd), _ = both_routes(b)
    seqs = set()
    for i, s in enumerate(b.sums):
        if s[28] == 0:
            assert fd[i]
            continue
        T, info = R.solve_666(R.sums_to_A(s[:21]), s[21:27])
        assert not fd[i] and same_bits(Ed[i].reshape(16), T), (i, b.tags[i], info.pivots)
        seqs.add(info.pivots)
    assert len(seqs) == 720


def test_device_iteration_logic_edges(batches):
    """cnt == 0, it == max_iteration, |dfitness| / |drmse| exactly at the threshold, thresholds 0 and inf, n_points 1 and around
    2^24, random (err, cnt, n): the same flags and values on both routes, and the flags the iteration logic prescribes."""
    want = {"cnt0": 3, "max-iter": 2, "max-iter-0": 2, "df-equal": 0, "df-below": 2, "dr-equal": 0, "dr-below": 1, "thr-0": 0,
            "thr-inf": 1, "n-edge": 7, "scores": 10000}
    for b in batches:
        if b.name not in want:
            continue
        (sd, Ed, fd), (sh, Eh, fh) = both_routes(b)
        assert int(fd.sum()) == want[b.name], b.name
        assert np.array_equal(fd, fh), b.name
        assert same_bits(sd["fitness"], sh["fitness"]) and same_bits(sd["inlier_rmse"], sh["inlier_rmse"]), b.name
        assert same_bits(sd["T"], sh["T"]) and same_bits(Ed, Eh), b.name
    cnt0 = next(b for b in batches if b.name == "cnt0")
    sd, _, _ = both_routes(cnt0)[0]
    assert np.all(sd["fitness"] == 0.5) and np.all(sd["inlier_rmse"] == 0.25)         # a hypothesis with no inlier keeps its scores


def test_device_solve_against_float64_truth(batches):
    b = batches[0]
    (sd, Ed, fd), _ = both_routes(b)
    for i in spd_rows(b):
        Tt, kappa, x = float64_truth(b.sums[i])
        assert np.all(np.abs(Ed[i].astype(np.float64) - Tt) <= truth_bound(Tt, kappa, x)), (i, b.tags[i], kappa)


def test_icp_realistic_systems_through_both_routes(batches):
    """The oracle's canonical 29-sum traces of configs[1] and configs[2] hypotheses, with the prior T the trace had reached."""
    b = batches[0]
    rows = [i for i, t in enumerate(b.tags) if t.startswith("icp-")]
    assert len(rows) >= 150
    sub = R.Batch("icp", b.sums[rows], b.n_points[rows], T=batches[1].T[:1].repeat(len(rows), 0), tags=[b.tags[i] for i in rows])
    (sd, Ed, fd), (sh, Eh, fh) = both_routes(sub)
    assert not fd.any() and np.array_equal(fd, fh)
    assert same_bits(Ed, Eh) and same_bits(sd["T"], sh["T"])
