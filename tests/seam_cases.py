"""The launch seam -- TEST INFRASTRUCTURE.  Every launch that puts the hypothesis index on grid.y runs in pieces of at most 32768 hypotheses, each
with its own ``+ p0`` on every array indexed by hypothesis.  A batch that repeats n inputs as ``i % n`` cannot see a dropped offset on anything
a piece READS when n divides 32768: hypothesis 32768 + j then has the input, and the answer, of hypothesis j.  ``seam_index`` steps the
repetition by one behind every seam, so that hypothesis SEAM + j never has the input of hypothesis j; ``assert_seam_visible`` states, on the
reference alone, that the expected rows do differ where the scheme needs them to."""
import functools

import numpy as np

SEAM = 32768
P = SEAM + 5
SPLIT_K = np.array([60.0, 0, 23.5, 0, 60.0, 15.5, 0, 0, 1], np.float32)      # the pinhole of verify_ref.launch_split_case's proj


def seam_index(P, n, seam=SEAM):
    """Which of n inputs hypothesis i takes: i % n before the seam, the next one behind it.  Hypothesis seam + j takes input (j + seam + 1) % n,
    which is not hypothesis j's whenever n does not divide seam + 1; neighbours still take neighbouring inputs, the pair across the seam two apart."""
    i = np.arange(P)
    return (i + i // seam) % n


def byte_rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def assert_records_take(got, want, idx, seam=SEAM):
    """got[i] == want[idx[i]] for every i, byte for byte: one comparison over the whole batch (verify_ref.assert_records_repeat with an explicit
    index).  The message names the first differing hypotheses and whether each lies behind the seam."""
    idx = np.asarray(idx)
    assert len(got) == len(idx), (len(got), len(idx))
    g, w = byte_rows(got), byte_rows(want)
    assert g.shape[1] == w.shape[1], (g.shape, w.shape)
    bad = np.flatnonzero((g != w[idx]).any(1))
    assert len(bad) == 0, (f"{len(bad)} of {len(idx)} records differ", [(int(i), "behind the seam" if i >= seam else "before the seam", "takes", int(idx[i]))
                                                                          for i in bad[:10]], got[bad[:3]], np.asarray(want)[idx[bad[:3]]])


def assert_seam_visible(want, idx, seam=SEAM, n_behind=5):
    """The condition the scheme rests on, on the reference alone: for j in 0 .. n_behind - 1 the rows want[idx[seam + j]] and want[idx[j]] differ in
    bytes (a piece that reads hypothesis j's input for seam + j gives another record), and so do the rows either side of the seam."""
    idx = np.asarray(idx)
    w = byte_rows(want)
    assert len(idx) >= seam + n_behind and idx.max() < len(w), (len(idx), seam, len(w))
    for j in range(n_behind):
        assert idx[seam + j] != idx[j] and (w[idx[seam + j]] != w[idx[j]]).any(), ("hypothesis", seam + j, "expects the record of hypothesis", j)
    assert (w[idx[seam - 1]] != w[idx[seam]]).any(), "the records either side of the seam are equal"
    assert set(idx[:seam].tolist()) == set(range(len(w))), "an input that does not occur before the seam"


def mesh_runs(P, n_meshes=2, run=5):
    """The mesh index of a mixed batch in runs of `run`: 32768 % 5 = 3, so a run straddles the seam."""
    return ((np.arange(P) // run) % n_meshes).astype(np.uint32)


def small_mesh(tris):
    return np.ascontiguousarray(np.asarray(tris, np.float32) * np.float32(0.8))


PYR2 = ((2, (0, 0, 2)), (1, (0, 0, 1)))                            # crosses the count and emit seams at P hypotheses
PYR4 = ((4, (0, 0, 1)), (3, (0, 0, 1)), (2, (0, 0, 1)), (1, (0, 0, 1)))      # 8200 hypotheses x 4 levels: the row scan's seam alone
SCAN_P = 8200
SCAN_SEAM = SEAM - 3 * SCAN_P                                      # (level, hypothesis) image 32768 is hypothesis 8168 of the last level
CRIT = (0.0, 0.0, 3)


@functools.lru_cache(maxsize=None)
def oracle_scenes():
    """The split case's scene as the CPU oracle's projective and kd-tree scene."""
    import oracle_lib as O
    from verify_ref import launch_split_case
    c = launch_split_case()
    return dict(proj=O.ProjScene(c["scene"], SPLIT_K), nn=O.NNScene(c["scene"], SPLIT_K))


@functools.lru_cache(maxsize=None)
def refine_ref(kind, ppb=2048, small=False):
    """(records[8], cloud sizes[8]) of the CPU oracle's refine_batch at CRIT on the split case's eight poses; `small`: the 0.8-scaled box."""
    import oracle_lib as O
    from verify_ref import launch_split_case
    c = launch_split_case()
    tris = small_mesh(c["tris"]) if small else c["tris"]
    res, sizes, _ = O.refine_batch(tris, c["poses"], c["W"], c["H"], c["proj"], SPLIT_K, oracle_scenes()[kind], CRIT, O.SUM_CANONICAL, ppb)
    return res, sizes


@functools.lru_cache(maxsize=None)
def pyramid_ref_records(kind, levels=PYR2, ppb=2048, small=False):
    """(records[8], level records[L, 8], level sizes[L, 8]) of pyramid_ref.refine_pyramid on the split case's eight poses."""
    import pyramid_ref
    from verify_ref import launch_split_case
    c = launch_split_case()
    tris = small_mesh(c["tris"]) if small else c["tris"]
    return pyramid_ref.refine_pyramid(tris, c["poses"], c["W"], c["H"], c["proj"], SPLIT_K, oracle_scenes()[kind], levels, ppb)


def split_clouds():
    """The eight emitted clouds of the split case (metres), as the fused path emits them: row-major over the render."""
    import oracle_lib as O
    from verify_ref import launch_split_case
    c = launch_split_case()
    return [O.depth2cloud(r, SPLIT_K) for r in c["renders"]]


@functools.lru_cache(maxsize=None)
def device_scenes():
    """The split case's scene on the device (api.init done by the caller): projective, kd-tree, and a closest-point grid of the kd-tree scene
    with its host copy (grid_ref's descriptor, cells, records) for the reference loop."""
    import grid_ref
    from pose_refine_amd import api
    from verify_ref import launch_split_case
    c = launch_split_case()
    proj = api.Scene_projective().init_Scene_projective_cuda(c["scene"], SPLIT_K, c["W"], c["H"])
    nn = api.Scene_nn().init_Scene_nn_cuda(c["scene"], SPLIT_K)
    grid = api.Scene_grid.from_scene_nn(nn, 0.008)
    host = (grid_ref.from_ctypes(grid.desc()), grid.cell_points().reshape(-1), grid.records())
    return dict(proj=proj, nn=nn, grid=grid, grid_host=host)


def seam_report(what, sizes, rows, idx, seam=SEAM):
    """Printed before the comparison: the cloud sizes of the inputs and the first bytes' worth of figures either side of the seam."""
    print(what, "cloud sizes of the inputs", np.asarray(sizes).tolist(), "| hypotheses", seam - 1, seam, "take", int(idx[seam - 1]), int(idx[seam]),
          "| rows", rows[seam - 1], rows[seam])


def mixed_table(per_mesh, mesh_index, idx):
    """For a mixed batch over the split case: the stacked single-mesh tables (mesh 0's rows, then mesh 1's ...) and the row each hypothesis takes."""
    n = len(per_mesh[0])
    return np.concatenate([byte_rows(t) for t in per_mesh]), np.asarray(mesh_index, np.int64) * n + np.asarray(idx, np.int64)


def pyramid_rows(out):
    """refine_pyramid's (records[P], level records[L, P], level sizes[L, P]) as one (P, bytes) table: a hypothesis' whole output in one row."""
    res, lres, lsizes = out
    n = len(res)
    return np.concatenate([byte_rows(res)] + [byte_rows(lres[l]) for l in range(len(lres))] + [byte_rows(np.ascontiguousarray(lsizes.T))], axis=1).reshape(n, -1)


def refine_rows(out):
    """refine_batch's (records[P], sizes[P]) as one (P, bytes) table."""
    res, sizes = out
    return np.concatenate([byte_rows(res), byte_rows(np.ascontiguousarray(sizes, np.uint32))], axis=1)
