"""The spatial order of the library's copy of a triangle buffer (pr_debug_mesh_order) and the order-independent fingerprint that guards it
(pr_debug_mesh_fingerprint): host code, no device.  And the claim the ordered copy rests on, counted with tools/raster_atomic_shape.py:
the raster's depth atomics address far fewer 64-byte segments per wave instruction when neighbours in the buffer are neighbours in space."""
import os
import sys

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import random_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import raster_atomic_shape as shape  # noqa: E402


def is_permutation(perm, n):
    return perm.dtype == np.uint32 and perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32))


def soup(n, seed=3):
    if n < 4:                                           # random_mesh plants its degenerate triangles in the first four places
        return np.random.default_rng(seed).normal(size=(n, 3, 3)).astype(np.float32)
    return random_mesh(np.random.default_rng(seed), n, 50.0)


def test_obj06_order_is_a_deterministic_permutation(obj06_tris):
    perm = api.mesh_order(obj06_tris)
    assert is_permutation(perm, len(obj06_tris))
    assert np.array_equal(perm, api.mesh_order(obj06_tris.copy()))
    assert not np.array_equal(perm, np.arange(len(perm)))          # the file has no spatial order: something moves


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_order_of_random_soups(n):
    tris = soup(n)
    perm = api.mesh_order(tris)
    assert is_permutation(perm, n)
    assert np.array_equal(perm, api.mesh_order(tris))


def test_equal_centroids_keep_index_order():
    tris = np.repeat(soup(1), 300, axis=0)                                 # 300 copies of one triangle
    assert np.array_equal(api.mesh_order(tris), np.arange(300, dtype=np.uint32))


def test_non_finite_triangles_go_last_in_index_order():
    tris = soup(1000)
    bad = [3, 17, 400, 999]
    tris[3, 0, 0] = np.nan
    tris[17, 2, 1] = np.inf
    tris[400, 1, 2] = -np.inf
    tris[999] = np.nan
    perm = api.mesh_order(tris)
    assert is_permutation(perm, 1000)
    assert perm[-4:].tolist() == bad
    # the finite ones are ordered as if the others were not there (they do not stretch the box the codes are taken in)
    keep = np.setdiff1d(np.arange(1000), bad)
    assert np.array_equal(keep[api.mesh_order(tris[keep])], perm[:-4])


def test_order_follows_space():
    """Triangles on a line, shuffled, fewer than the 1024 cells of an axis: the order walks the line (a Morton code along one axis is monotonic)."""
    rng = np.random.default_rng(2)
    x = rng.permutation(1000).astype(np.float32)
    tris = np.zeros((1000, 3, 3), np.float32)
    tris[:, :, 0] = x[:, None]
    tris[:, 1, 1] = 0.25
    tris[:, 2, 2] = 0.25
    assert np.all(np.diff(x[api.mesh_order(tris)]) > 0)


def test_fingerprint_is_a_multiset_hash(obj06_tris):
    fp = api.mesh_fingerprint(obj06_tris)
    perm = api.mesh_order(obj06_tris)
    assert api.mesh_fingerprint(obj06_tris[perm]) == fp
    assert api.mesh_fingerprint(obj06_tris[::-1]) == fp
    assert api.mesh_fingerprint(obj06_tris[:0]) == 0
    rng = np.random.default_rng(11)
    for _ in range(32):                                             # one word of one triangle, by one unit in the last place
        t, w = int(rng.integers(len(obj06_tris))), int(rng.integers(9))
        other = obj06_tris.copy()
        bits = other.reshape(-1, 9).view(np.uint32)
        bits[t, w] ^= np.uint32(1)
        assert api.mesh_fingerprint(other) != fp
    # the words of a triangle are not interchangeable, nor are triangles that swap single vertices
    other = obj06_tris.copy()
    other[7] = other[7][[1, 0, 2]]
    assert api.mesh_fingerprint(other) != fp
    other = obj06_tris.copy()
    other[[7, 8], 0] = other[[8, 7], 0]
    assert api.mesh_fingerprint(other) != fp


def test_shipped_order_needs_at_most_0_6_of_the_atomic_requests_of_file_order():
    """On the first 6 benchmark hypotheses: 64-byte atomic requests per hypothesis, the sum over the raster's atomic wave instructions of
    the distinct segments their lanes address.  File order is 1.0 by definition; a Morton order of the centroids gives 0.47 (14 212
    against 30 550).  The cap leaves room for another order and none for no order."""
    tris = shape.load_obj06()
    poses = synth.hypotheses(6)
    file_order = shape.requests_per_hypothesis(tris, poses)
    shipped = shape.requests_per_hypothesis(shape.shipped_order(tris), poses)
    print(f"64-B requests per hypothesis: file order {file_order:.0f}, shipped order {shipped:.0f}, ratio {shipped / file_order:.3f}")
    assert shipped <= 0.6 * file_order
