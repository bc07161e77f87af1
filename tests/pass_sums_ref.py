"""Inputs and oracle traces shared by test_pass_sums_host.py and test_pass_sums_gpu.py: windows of the scenario cloud taken where the scene
is, so that every size keeps inliers, and the canonical-tree sums of every pass of the CPU oracle on them (computed once per window, tree and
criteria, then shared read-only)."""
import numpy as np

import oracle_lib as O

WINDOW_START = 12001          # an odd point index inside the part of the scenario cloud that projects onto the scene
# around every width the pass is built from: one point, a partial wavefront, 64 / 256 / 1024 (wavefront, workgroup, point step), 3072 (the default
# points_per_block), two workgroups, and 16 / 17 workgroups of 1024 (sum_partials adds workgroup sums in chunks of 16)
SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073, 6143, 6144, 6145, 16384, 16385)
NN_SIZES = (1, 5, 64, 65, 257, 1025, 3073, 6145)
PPBS = (1024, 3072, 65536)


def window(cloud, n):
    """n points of the cloud from WINDOW_START; a window longer than what is left behind WINDOW_START ends at the cloud's end instead (16 384 and
    16 385 points of the 26 210: starts 9826 and 9825), so that its size is what it says."""
    start = min(WINDOW_START, len(cloud) - n)
    assert start >= 0, (n, len(cloud))
    w = cloud[start:start + n]
    assert len(w) == n
    return w


def sizes_for(ppb, cloud_len):
    """SIZES plus the 16 / 17-workgroup boundary of this points_per_block where the cloud is long enough (16 384 / 16 385 for 1024: already in SIZES)."""
    extra = [n for n in (16 * ppb, 16 * ppb + 1) if n <= cloud_len and n not in SIZES]
    return list(SIZES) + extra


def odd_start_order(sizes):
    """The sizes reordered so that, concatenated from point 0, as many parts as possible start at an odd point index: a part that starts at an
    odd index and has an even size keeps the next start odd, so even sizes are spent while the start is odd and odd sizes while it is even."""
    even = sorted((n for n in sizes if n % 2 == 0), reverse=True)
    odd = sorted((n for n in sizes if n % 2 == 1), reverse=True)
    out, at = [], 0
    while even or odd:
        if at % 2 == 1:
            pick = even.pop() if even else odd.pop()
        else:
            pick = odd.pop() if odd else even.pop()
        out.append(pick)
        at += pick
    return out


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing_columns(a, b):
    return int((u32(a) != u32(b)).sum())


_traces = {}


def oracle_trace(cloud, scene, crit, ppb):
    """(record, passes, (passes, 29) canonical-tree sums) of O.icp on `cloud`; cached by content, scene object, criteria and tree."""
    cl = np.ascontiguousarray(cloud, np.float32)
    key = (cl.tobytes(), id(scene), tuple(crit), int(ppb))
    hit = _traces.get(key)
    if hit is None:
        rec, passes, _, tr = O.icp(cl, scene, tuple(crit), O.SUM_CANONICAL, int(ppb), trace=True)
        tr.setflags(write=False)
        hit = _traces[key] = (rec.copy(), passes, tr, scene)          # (the scene is held so that its id stays its own)
    return hit[0], hit[1], hit[2]


def expect_rows(n_passes, clouds, scene, crit, ppb):
    """The (n_passes, len(clouds), 29) array a trace of the batch must equal, bit for bit: NaN where the library may not write (an empty cloud, the
    passes after a hypothesis has finished), the oracle's sums elsewhere.  Returns it with the oracle's records and pass counts."""
    want = np.full((n_passes, len(clouds), 29), np.nan, np.float32)
    recs, passes = [], []
    for i, cl in enumerate(clouds):
        if len(cl) == 0:
            recs.append(None); passes.append(0)
            continue
        rec, p, tr = oracle_trace(cl, scene, crit, ppb)
        want[:p, i] = tr
        recs.append(rec); passes.append(p)
    return want, recs, passes
