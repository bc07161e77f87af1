"""The host 6x6 update solver and the host-solve loop's iteration, held to tests/solve_ref.py (a bit-exact Python restatement) and to
a float64 truth, over a corpus that reaches all 720 pivot sequences and every branch edge of the solver (CPU only: the host route of
pr_debug_pose_iteration and pr_solve_666 need no device)."""
import collections
import math

import numpy as np
import pytest

import solve_ref as R
from pose_refine_amd import api
from truth_ref import float64_truth


@pytest.fixture(scope="module")
def batches(scenario):
    return R.solve_batches(scenario) + R.iteration_batches()


@pytest.fixture(scope="module")
def solve_batch(batches):
    return batches[0]


@pytest.fixture(scope="module")
def infos(solve_batch):
    return [R.solve_666(R.sums_to_A(s[:21]), s[21:27]) for s in solve_batch.sums]


def same_bits(a, b):
    """Bit for bit, NaN where the other is NaN (NaN payloads and signs are not compared)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def test_corpus_reaches_all_720_pivot_sequences(solve_batch, infos):
    seqs = collections.defaultdict(set)
    for tag, (_, info) in zip(solve_batch.tags, infos):
        seqs[tag].add(info.pivots)
    every = set(R.ALL_PIVOT_SEQUENCES())
    assert len(every) == 720
    print(f"\npivot sequences covered: diagonal family {len(seqs['pivot-diag'])}/720, random SPD {len(seqs['pivot-spd'])}/720, "
          f"whole corpus {len(set().union(*seqs.values()))}/720")
    assert seqs["pivot-diag"] == every
    assert seqs["pivot-spd"] == every
    assert sum(t == "pivot-spd" for t in solve_batch.tags) == 3 * 720
    assert len(seqs["icp-proj"]) >= 1 and len(seqs["icp-nn"]) >= 1


def test_corpus_hits_every_branch_edge(solve_batch, infos):
    by = collections.defaultdict(list)
    for tag, (_, info) in zip(solve_batch.tags, infos):
        by[tag].append(info)
    assert sum(i.ties > 0 for i in by["tie"]) == len(by["tie"]) >= 2
    assert sum(i.ties > 0 for i in by["tie-sign"]) == len(by["tie-sign"]) >= 2
    assert len(by["zero"]) == 2 and all(i.pivots == (0, 1, 2, 3, 4, 5) for i in by["zero"])
    for rank in range(1, 6):
        assert len(by[f"rank{rank}"]) == 2
    assert len(by["indefinite"]) == 4
    assert sum(i.dk_zero for i in by["dk0"]) >= 2 and sum(i.tiny for i in by["dk0"]) >= 2       # dk == 0 undivided column, pseudo-inverse
    assert len(by["dk-small"]) == 1 and len(by["b0"]) == 1 and len(by["huge"]) == 2 and len(by["denormal"]) == 3
    branches = collections.Counter(b for info in by["angle"] for b in info.sincos)
    assert branches["kernel"] >= 3 and branches["reduced"] >= 10 and branches["cut"] >= 5, branches
    halves = [abs(info.half_angles[0]) for info in by["angle"]]
    assert any(0 < h <= R.QUARTER_PI and R.QUARTER_PI - h < 1e-7 for h in halves)          # the float32 neighbours of pi/4, both sides
    assert any(h > R.QUARTER_PI and h - R.QUARTER_PI < 1e-7 for h in halves)
    assert any(math.isnan(h) for h in halves) and any(h >= 1e9 for h in halves) and any(1e8 < h < 1e9 for h in halves)
    assert len(by["nonfinite-A"]) == 4 and len(by["nonfinite-b"]) == 3
    assert sum(len(v) for k, v in by.items() if k.startswith("icp-")) >= 150


def test_restatement_equals_pr_solve_666_bitwise(solve_batch, infos):
    """tests/solve_ref.py is the same computation as the host solver (pr_solve_666), bit for bit, over the whole corpus."""
    bad = []
    for i, (s, (T, _)) in enumerate(zip(solve_batch.sums, infos)):
        H = api.eigen_slover_666(R.sums_to_A(s[:21]), s[21:27]).reshape(16)
        if not same_bits(H, T):
            bad.append((i, solve_batch.tags[i]))
    assert not bad, bad[:10]


def run_restatement(b):
    out_T, out_r, out_f, out_E, out_fin = [], [], [], [], []
    for i in range(len(b.sums)):
        T, rmse, fit, E, _ = R.pose_iteration(b.sums[i], int(b.n_points[i]), b.T[i], b.rmse[i], b.fitness[i], b.crit, b.it)
        out_T.append(T); out_r.append(rmse); out_f.append(fit)
        out_E.append(np.zeros(16, np.float32) if E is None else E); out_fin.append(E is None)
    return (np.array(out_T, np.float32), np.array(out_r, np.float32), np.array(out_f, np.float32), np.array(out_E, np.float32),
            np.array(out_fin))


def state_of(b):
    st = np.zeros(len(b.sums), api.RESULT)
    st["T"] = b.T
    st["inlier_rmse"] = b.rmse
    st["fitness"] = b.fitness
    return st


def test_host_iteration_equals_restatement(batches):
    """pr_debug_pose_iteration's host route (the host-solve loop's pose_iteration_host) against the restatement: the new T, rmse,
    fitness, E and the finished flag, bit for bit, on every batch (solve corpus, non-identity priors and the iteration-logic edges)."""
    seen = collections.Counter()
    for b in batches:
        st, E, fin = api.debug_pose_iteration(b.sums, b.n_points, api.ICPConvergenceCriteria(*b.crit), b.it, False, state_of(b))
        T, rmse, fit, Er, finr = run_restatement(b)
        assert np.array_equal(fin, finr), b.name
        assert same_bits(st["T"], T), b.name
        assert same_bits(st["inlier_rmse"], rmse) and same_bits(st["fitness"], fit), b.name
        assert same_bits(E.reshape(-1, 16), Er), b.name
        seen[b.name] = int(fin.sum())
    # the iteration-logic edges stop where they must
    assert seen["cnt0"] == 3 and seen["max-iter"] == 2 and seen["max-iter-0"] == 2 and seen["scores"] == 10000
    assert seen["df-equal"] == 0 and seen["df-below"] == 2 and seen["dr-equal"] == 0 and seen["dr-below"] == 1
    assert seen["thr-0"] == 0 and seen["thr-inf"] == 1 and seen["n-edge"] == 7               # a NaN rmse never counts as converged
    nonzero_cnt = batches[0].sums[:, 28] != 0
    assert seen["solve"] == int((~nonzero_cnt).sum())


def truth_bound(Tt, kappa, x):
    """1 float32 ulp of the float64 entry when kappa(A + 0.01 I) <= 1e6; above that, plus kappa * 2^-52 times the entry's scale
    (1 for the rotation, max |x| for the translation)."""
    ulp = np.spacing(np.abs(Tt).astype(np.float32)).astype(np.float64)
    if kappa <= 1e6:
        return ulp
    scale = np.ones((4, 4))
    scale[:3, 3] = np.abs(x).max()
    return ulp + kappa * 2.0 ** -52 * scale


def spd_rows(batch):
    return [i for i, t in enumerate(batch.tags) if t in ("pivot-diag", "pivot-spd", "icp-proj", "icp-nn")]


def test_host_solve_against_float64_truth(solve_batch):
    n_well = 0
    for i in spd_rows(solve_batch):
        s = solve_batch.sums[i]
        T = api.eigen_slover_666(R.sums_to_A(s[:21]), s[21:27]).astype(np.float64)
        Tt, kappa, x = float64_truth(s)
        assert np.all(np.abs(T - Tt) <= truth_bound(Tt, kappa, x)), (i, solve_batch.tags[i], kappa, np.abs(T - Tt).max())
        n_well += kappa <= 1e6
    assert n_well >= 1500


def test_sincos_accuracy():
    """sincos_d: < 1 ulp on |x| <= pi/4 (the polynomial alone); beyond, after the Cody-Waite reduction, within 1 ulp(1.0) of
    math.sin / math.cos up to the 1e9 cut-off (the former two-piece reduction was off by up to 2.7e8 ulp(1.0) above 1e7)."""
    rng = np.random.default_rng(3)
    q = R.QUARTER_PI
    small = np.concatenate([rng.uniform(-q, q, 20000), [0.0, q, -q, np.nextafter(q, 0), 1e-300, 5e-324, 1e-8]])
    for x in small:
        s, c = R.sincos_d(float(x))
        assert abs(s - math.sin(x)) <= np.spacing(abs(math.sin(x))) and abs(c - math.cos(x)) <= np.spacing(abs(math.cos(x))), x
    big = np.concatenate([10.0 ** rng.uniform(math.log10(q), 9, 20000) * rng.choice([-1.0, 1.0], 20000),
                          [np.nextafter(q, 1), math.pi / 2, math.pi, 1e3, 1e5, 1e7, np.nextafter(1e9, 0), -np.nextafter(1e9, 0),
                           2 ** 29 * math.pi, 6.4e8 * math.pi / 2]])
    ulp1 = 2.0 ** -52
    for x in big:
        x = float(x)
        if abs(x) >= 1e9:
            continue
        s, c = R.sincos_d(x)
        assert abs(s - math.sin(x)) <= ulp1 and abs(c - math.cos(x)) <= ulp1, x
    assert R.sincos_d(1e9) == (0.0, 1.0) and R.sincos_d(math.nan) == (0.0, 1.0) and R.sincos_d(-math.inf) == (0.0, 1.0)
