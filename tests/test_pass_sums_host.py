"""The inputs of test_pass_sums_gpu.py have teeth (no GPU; the CPU oracle only): on the windows of the scenario cloud that file compares bit for
bit, every size keeps inliers on both scenes, the canonical tree differs from the sequential sum in many of the 29 columns, and the tree of one
points_per_block differs from another's.  A reduction that added the right terms in another order would therefore not go unnoticed there.  These
are conditions on the INPUTS: if a change of the fixtures breaks one, another window is the cure, not a lower bound."""
import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib
from pass_sums_ref import NN_SIZES, PPBS, SIZES, differing_columns, odd_start_order, sizes_for, window

ALL_SIZES = sorted({n for ppb in PPBS for n in sizes_for(ppb, 26210)})


@pytest.fixture(scope="module")
def rows(scenario):
    """Canonical (ppb 3072 and 1024) and sequential rows of every window, on both scenes; kd-tree rows only for the sizes that scene is run at."""
    cloud = scenario["cloud"]
    assert len(cloud) == 26210
    out = {}
    for kind, scene, sizes in (("proj", scenario["proj_scene"], ALL_SIZES), ("nn", scenario["nn_scene"], NN_SIZES)):
        for n in sizes:
            w = window(cloud, n)
            out[kind, n] = dict(canon=O.sum29(w, scene, O.SUM_CANONICAL, 3072), canon1024=O.sum29(w, scene, O.SUM_CANONICAL, 1024),
                                seq=O.sum29(w, scene, O.SUM_SEQUENTIAL))
    return out


def test_size_lists(scenario):
    n = len(scenario["cloud"])
    assert sizes_for(3072, n) == list(SIZES)                       # 49 152 points: longer than the cloud
    assert sizes_for(1024, n) == list(SIZES)                       # 16 384 / 16 385 are in the list
    assert sizes_for(65536, n) == list(SIZES)
    for n_pts in (16384, 16385):
        assert len(window(scenario["cloud"], n_pts)) == n_pts
    order = odd_start_order(list(SIZES) + [0])
    assert sorted(order) == sorted(list(SIZES) + [0])
    starts = np.cumsum([0] + order[:-1])
    # most parts of the ragged batch start at an odd point index (15 of 22 is the most any order gives: each of the 14 odd sizes flips the parity)
    assert (starts % 2 == 1).sum() == 15, starts
    assert {1, 3} <= set(int(v) for v in starts % 4)               # ... of both residues a 16-byte load cares about


def test_every_window_keeps_inliers(rows):
    for (kind, n), r in rows.items():
        assert r["canon"][28] > 0, (kind, n)
        if kind == "nn":
            assert r["canon"][28] == n, n                          # every point of a window has a neighbour within reach
        elif n >= 63:
            assert r["canon"][28] >= 53, n


def test_canonical_tree_differs_from_the_sequential_sum(rows):
    for (kind, n), r in rows.items():
        if n >= 63:
            assert differing_columns(r["canon"], r["seq"]) >= 10, (kind, n, differing_columns(r["canon"], r["seq"]))


def test_trees_of_different_points_per_block_differ(rows):
    for (kind, n), r in rows.items():
        if n > 1024:
            assert differing_columns(r["canon"], r["canon1024"]) >= 6, (kind, n, differing_columns(r["canon"], r["canon1024"]))
        else:
            assert differing_columns(r["canon"], r["canon1024"]) == 0, (kind, n)     # one point step: the same tree


def test_recorder_disarms_without_a_device():
    assert _lib.load().pr_debug_trace_sums(None, 0, 0) == _lib.PR_OK
