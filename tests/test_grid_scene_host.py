"""The closest-point grid scene (pr_scene_grid) without a device: pr_scene_grid_describe against tests/grid_ref.py, its refusals, the struct's
layout and the ABI version, and grid_ref itself against a float64 restatement of what the grid approximates (the header's bound)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grid_ref
import truth_ref
from pose_refine_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def describe(lo, hi, cell, mdd=0.01, reach=0.02):
    d = _lib.SceneGridDesc()
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    rc = _lib.load().pr_scene_grid_describe(lo.ctypes.data, hi.ctypes.data, C.c_float(cell), C.c_float(mdd), C.c_float(reach), C.addressof(d))
    return rc, d


# lo, hi, cell: a flat axis (dim 1), a cell that does not divide the extent, negative origins, a single cell, extents that are exact multiples of the
# cell (hi must still be inside), a cell larger than the box, tiny and huge coordinates, one long axis
BOXES = [
    ((0, 0, 0), (1, 1, 1), 0.25),
    ((-0.3, -0.2, 0.4), (0.3, 0.2, 0.4), 0.002),
    ((-0.3, -0.2, 0.4), (0.3, 0.2, 0.9), 0.007),
    ((-1.5, -2.5, -3.5), (-1.0, -2.0, -3.0), 0.013),
    ((0.1, 0.1, 0.1), (0.1, 0.1, 0.1), 0.001),
    ((0, 0, 0), (0.5, 0.25, 0.125), 0.125),
    ((0, 0, 0), (0.001, 0.001, 0.001), 1.0),
    ((-0.064, -0.064, 0.5), (0.064, 0.064, 0.628), 0.004),
    ((1e-6, -1e-6, 0), (3e-6, 1e-6, 1e-6), 1e-7),
    ((1000, 2000, 3000), (1000.5, 2000.25, 3000.125), 0.03125),
    ((0, 0, 0), (60.0, 0.01, 0.01), 0.001),
    ((-0.123456, 0.2345678, 0.3456789), (0.4567891, 0.5678912, 0.6789123), 0.00317),
]


@pytest.mark.parametrize("lo,hi,cell", BOXES)
def test_describe_matches_the_reference(lo, hi, cell):
    rc, d = describe(lo, hi, cell, 0.01, 0.0125)
    assert rc == _lib.PR_OK, _lib.load().pr_last_error()
    want = grid_ref.describe(lo, hi, cell, 0.01, 0.0125)
    got = grid_ref.from_ctypes(d)
    assert got.dim == want.dim and min(got.dim) >= 1 and np.prod([float(v) for v in got.dim]) <= _lib.GRID_MAX_CELLS
    assert np.array_equal(got.origin.view(np.uint32), want.origin.view(np.uint32))
    for f in ("cell", "inv_cell", "max_dist_diff", "reach"):
        assert F32(getattr(got, f)).view(np.uint32) == F32(getattr(want, f)).view(np.uint32), f
    assert got.inv_cell == F32(1.0) / F32(cell)
    assert d.n_points == 0 and not d.cell_point and not d.rec
    # both corners of the box are inside the grid it describes, lo in cell 0
    inside, idx = grid_ref.cell_of(np.array([lo, hi], F32), got)
    assert inside.all() and idx[0] == 0 and idx[1] == np.prod(got.dim) - 1


def test_flat_axis_has_one_cell():
    rc, d = describe((-0.25, -0.125, 0.5), (0.25, 0.125, 0.5), 1.0 / 512)      # (dyadic: the quotients are exact)
    assert rc == _lib.PR_OK and d.dim[2] == 1 and d.dim[0] == 257 and d.dim[1] == 129


REFUSED = [
    ("cell zero", (0, 0, 0), (1, 1, 1), 0.0, 0.01, 0.02),
    ("cell negative", (0, 0, 0), (1, 1, 1), -0.01, 0.01, 0.02),
    ("cell nan", (0, 0, 0), (1, 1, 1), np.nan, 0.01, 0.02),
    ("cell inf", (0, 0, 0), (1, 1, 1), np.inf, 0.01, 0.02),
    ("hi below lo", (0, 0, 0), (1, -1e-6, 1), 0.1, 0.01, 0.02),
    ("too many cells", (0, 0, 0), (1, 1, 1), 0.002, 0.01, 0.02),           # 501^3 > 2^26
    ("just too many cells", (0, 0, 0), (4.095, 4.095, 4.0), 0.01, 0.01, 0.02),   # 410 * 410 * 401 > 2^26
    ("a dim that overflows", (0, 0, 0), (1e9, 0, 0), 1e-3, 0.01, 0.02),
    ("an extent that overflows", (-3e38, 0, 0), (3e38, 0, 0), 1.0, 0.01, 0.02),
    ("lo nan", (np.nan, 0, 0), (1, 1, 1), 0.1, 0.01, 0.02),
    ("radius zero", (0, 0, 0), (1, 1, 1), 0.1, 0.0, 0.02),
    ("reach nan", (0, 0, 0), (1, 1, 1), 0.1, 0.01, np.nan),
]


@pytest.mark.parametrize("what,lo,hi,cell,mdd,reach", REFUSED)
def test_describe_refuses(what, lo, hi, cell, mdd, reach):
    rc, _ = describe(lo, hi, cell, mdd, reach)
    assert rc == _lib.PR_ERR_INVALID, what
    assert len(_lib.load().pr_last_error()) > 0


def test_describe_accepts_the_largest_grid():
    rc, d = describe((0, 0, 0), (4.055, 4.055, 4.0), 0.01)          # 406 * 406 * 401 <= 2^26
    want = grid_ref.describe((0, 0, 0), (4.055, 4.055, 4.0), 0.01, 0.01, 0.02)
    assert rc == _lib.PR_OK and tuple(d.dim) == want.dim and np.prod(want.dim) <= _lib.GRID_MAX_CELLS


def test_null_arguments_are_refused():
    d = _lib.SceneGridDesc()
    lo = np.zeros(3, F32)
    lib = _lib.load()
    assert lib.pr_scene_grid_describe(None, lo.ctypes.data, C.c_float(0.1), C.c_float(0.1), C.c_float(0.1), C.addressof(d)) == _lib.PR_ERR_INVALID
    assert lib.pr_scene_grid_describe(lo.ctypes.data, lo.ctypes.data, C.c_float(0.1), C.c_float(0.1), C.c_float(0.1), None) == _lib.PR_ERR_INVALID
    assert len(lib.pr_last_error()) > 0


def test_abi_version_is_unchanged():
    assert _lib.load().pr_abi_version() == 4


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and the member offsets of pr_scene_grid as a C compiler sees the header, against the ctypes mirror."""
    fields = [f for f, _ in _lib.SceneGridDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pose_refine.h"\nint main(void) {\n  printf("%zu", sizeof(pr_scene_grid));\n'
                   + "".join(f'  printf(" %zu", offsetof(pr_scene_grid, {f}));\n' for f in fields)
                   + '  printf(" %d %u %u\\n", PR_SCENE_GRID, PR_GRID_NONE, PR_GRID_MAX_CELLS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.SceneGridDesc) == 64
    assert out[1:1 + len(fields)] == [getattr(_lib.SceneGridDesc, f).offset for f in fields]
    assert out[-3:] == [_lib.SCENE_GRID, _lib.GRID_NONE, _lib.GRID_MAX_CELLS]
    assert api.Scene_grid.kind == _lib.SCENE_GRID == 3


# ---- grid_ref against float64: what the grid approximates --------------------------------------------------------------------------
def _small_scene(seed=5):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-0.05, 0.05, 500), rng.uniform(-0.05, 0.05, 500), 0.4 + 0.01 * rng.normal(size=500)], 1).astype(F32)
    nrm = rng.normal(size=(500, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    return pts, nrm


def _host_grid(pts, nrm, desc):
    """A grid built on the host by the reference itself: the first point of every cell's tie set."""
    bf = grid_ref.expected_cells(desc, pts)
    cp = np.array([t[0] if ins else grid_ref.NONE for t, ins in zip(bf.ties, bf.inside)], np.uint32)
    rec = np.zeros((len(pts), 8), F32)
    rec[:, 0:3], rec[:, 4:7] = pts, nrm
    return cp, rec, bf


def test_reference_meets_the_bound_in_float64():
    """On 2 000 in-grid queries over a 500-point scene the grid's answer is never more than sqrt(3) * cell + 1e-6 farther than the true nearest
    point, and grid and truth agree on validity whenever the true distance is outside [max_dist_diff -+ sqrt(3) * cell]."""
    pts, nrm = _small_scene()
    cell, mdd = 0.004, 0.012
    reach = mdd + 0.5 * np.sqrt(3.0) * cell
    desc = grid_ref.describe(pts.min(0) - F32(mdd), pts.max(0) + F32(mdd), cell, mdd, reach)
    assert np.prod(desc.dim) <= 32 ** 3
    cp, rec, _ = _host_grid(pts, nrm, desc)
    rng = np.random.default_rng(6)
    lo = desc.origin.astype(np.float64)
    hi = lo + np.array(desc.dim) * float(desc.cell)
    q = rng.uniform(lo, hi, size=(2400, 3)).astype(F32)
    inside, _ = grid_ref.cell_of(q, desc)
    q = q[inside][:2000]
    assert len(q) == 2000
    winner, valid = grid_ref.associate(q, desc, cp, rec)
    d_all = np.linalg.norm(q.astype(np.float64)[:, None, :] - pts.astype(np.float64)[None, :, :], axis=2)
    true_d = d_all.min(1)
    slack = np.sqrt(3.0) * cell
    has = winner != grid_ref.NONE
    assert has.sum() > 500 and (~has).sum() > 100 and valid.sum() > 200
    got_d = d_all[np.arange(len(q)), np.where(has, winner, 0)]
    assert (got_d[has] <= true_d[has] + slack + 1e-6).all()
    # a NONE cell: the centre's nearest point is at least `reach` away, so the query's is farther than max_dist_diff - sqrt(3)/2 cell (within float32 rounding of reach)
    assert (true_d[~has] >= mdd - 1e-6).all()
    clear_in, clear_out = true_d < mdd - slack, true_d > mdd + slack
    assert clear_in.sum() > 50 and clear_out.sum() > 200
    assert valid[clear_in].all() and not valid[clear_out].any()


def test_reference_terms_match_float64_point_to_plane():
    pts, nrm = _small_scene(7)
    desc = grid_ref.describe(pts.min(0) - F32(0.01), pts.max(0) + F32(0.01), 0.005, 0.01, 0.015)
    cp, rec, _ = _host_grid(pts, nrm, desc)
    rng = np.random.default_rng(8)
    q = (pts[rng.integers(0, len(pts), 800)] + rng.normal(size=(800, 3)) * 0.003).astype(F32)
    w, v = grid_ref.associate(q, desc, cp, rec)
    assert 100 < v.sum() < 800
    t = grid_ref.terms29(q, w, v, rec)
    assert not t[~v].any() and (t[v, 28] == 1).all()
    want, scale = truth_ref.point_to_plane_terms(q[v], pts[w[v]], nrm[w[v]])
    assert (np.abs(t[v].astype(np.float64) - want) <= 8 * 2.0 ** -24 * scale).all()
    # the tree adds what it is given: integers stay exact, whatever the tree's shape
    ones = np.zeros((5000, 29), F32); ones[:, 28] = 1; ones[:, 0] = np.arange(5000) % 7
    for ppb in (1024, 3072):
        s = grid_ref.canonical_sums(ones, ppb)
        assert s[28] == 5000 and s[0] == (np.arange(5000) % 7).sum()


def test_cell_of_edges():
    desc = grid_ref.describe((0, 0, 0), (1, 1, 1), 0.25, 0.01, 0.02)
    assert desc.dim == (5, 5, 5)
    p = np.array([[0, 0, 0], [1.25, 0, 0], [np.nextafter(F32(1.25), F32(0)), 0, 0], [-1e-30, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0],
                  [0.25, 0.5, 0.75], [1e-40, 0, 0]], F32)
    inside, idx = grid_ref.cell_of(p, desc)
    assert inside.tolist() == [True, False, True, False, False, False, False, True, True]
    assert idx.tolist() == [0, 0, 4, 0, 0, 0, 0, 1 + 5 * (2 + 5 * 3), 0]
