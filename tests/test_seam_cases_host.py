"""Host tests of tests/seam_cases.py: the index, the two assertions, and -- on every reference table the GPU seam tests compare with -- the
condition the scheme rests on: the rows expected either side of the 32768-hypothesis seam differ, and hypothesis 32768 + j never expects
hypothesis j's row.  No GPU: the references alone."""
import numpy as np
import pytest

import seam_cases as S
from seam_cases import P, SEAM, assert_records_take, assert_seam_visible, seam_index
from verify_ref import launch_split_case


def test_index():
    assert (SEAM, P) == (32768, 32768 + 5) and launch_split_case()["P"] == P
    for n in (8, 32):
        idx = seam_index(P, n)
        assert np.array_equal(idx[:SEAM], np.arange(SEAM) % n) and idx[SEAM:].tolist() == [(j + 1) % n for j in range(5)]
        assert (idx[SEAM:] != idx[:5]).all() and set(idx[:SEAM].tolist()) == set(range(n))
        assert (np.bincount(idx, minlength=n) >= SEAM // n).all()
    idx = seam_index(S.SCAN_P, 8, S.SCAN_SEAM)                       # the row scan's seam: image 32768 of 4 levels x 8200 hypotheses
    assert S.SCAN_SEAM == 8168 and 3 * S.SCAN_P + S.SCAN_SEAM == SEAM and idx[8167] == 7 and idx[8168] == 1 and idx[8199] == 0
    runs = S.mesh_runs(P)
    assert runs[SEAM - 3:SEAM + 2].tolist() == [runs[SEAM]] * 5 and runs[SEAM - 4] != runs[SEAM] != runs[SEAM + 2]       # a run straddles the seam
    assert runs[:10].tolist() == [0] * 5 + [1] * 5


def test_assertions_see_what_they_are_for():
    want = np.arange(8 * 3, dtype=np.uint32).reshape(8, 3)
    idx = seam_index(P, 8)
    got = want[idx]
    assert_records_take(got, want, idx)
    assert_seam_visible(want, idx)
    # a second piece that read its inputs without its offset: hypothesis 32768 + j holds hypothesis j's record
    dropped = got.copy(); dropped[SEAM:] = got[:5]
    with pytest.raises(AssertionError, match="behind the seam"):
        assert_records_take(dropped, want, idx)
    with pytest.raises(AssertionError, match="before the seam"):
        assert_records_take(np.roll(got, 1, axis=0), want, idx)
    # ... which the plain repetition cannot see, and assert_seam_visible says so
    plain = np.arange(P) % 8
    assert_records_take(want[plain][np.r_[0:SEAM, 0:5]], want, plain)
    with pytest.raises(AssertionError):
        assert_seam_visible(want, plain)
    same = want.copy(); same[1] = same[0]                           # two equal reference rows where the scheme needs them to differ
    with pytest.raises(AssertionError):
        assert_seam_visible(same, idx)
    with pytest.raises(AssertionError):
        assert_records_take(got[:-1], want, idx)


def _fit_table(recs):
    from contour_fit_ref import FIT_FIELDS
    return np.array([[float(r[f]) for f in FIT_FIELDS] + list(np.asarray(r["sums"], np.float64)) for r in recs], np.float64)


def test_split_case_tables_differ_across_the_seam():
    import contour_fit_ref as CF
    from normals_ref import normals_ref
    from solid_ref import span_ref
    c = launch_split_case()
    idx = seam_index(P, 8)
    N = CF.nearest_ref(c["scene"], c["jump"], 3)
    cs = CF.centers(c["poses"], np.zeros(3, np.float32))
    fit = CF.fit_records(c["renders"], c["scene"], N, c["tau"], c["jump"], S.SPLIT_K, cs, 0.08)
    normals = normals_ref(c["renders"], c["scene"], c["tau"], S.SPLIT_K, 1, c["jump"], float(np.cos(np.deg2rad(30.0))))
    near, far = span_ref(c["tris"], c["poses"], c["proj"], c["W"], c["H"])
    tables = dict(poses=c["poses"], scores=c["scores"], contours=c["contours"], fit=_fit_table(fit), normals=normals, renders=c["renders"], far=far)
    assert np.array_equal(near, c["renders"])
    for what, t in tables.items():
        distinct = len({np.ascontiguousarray(r).tobytes() for r in t})
        assert len(t) == 8 and distinct == (7 if what == "normals" else 8), what        # (poses 5 and 7 have no inlier: all-zero normal records)
        assert_seam_visible(t, idx)
    assert not normals[5].tobytes().strip(b"\0") and not normals[7].tobytes().strip(b"\0")


def test_vsd_records_differ_across_the_seam():
    import vsd_ref as R
    c = R.small_case()
    want = R.vsd_ref(c["r_est"], c["r_gt"], c["scene"], c["K"], c["delta"], c["taus"])
    assert len(want) == 32 and len({r.tobytes() for r in want}) == 32
    assert_seam_visible(want, seam_index(P, 32))
    assert_seam_visible(np.concatenate([c["est"].reshape(32, -1), c["gt"].reshape(32, -1)], 1), seam_index(P, 32))


@pytest.mark.parametrize("small", [False, True], ids=["box", "box x 0.8"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_refinement_records_differ_across_the_seam(kind, small):
    res, sizes = S.refine_ref(kind, small=small)
    if not small:
        assert sizes.tolist() == [301, 394, 272, 176, 172, 123, 161, 670] == launch_split_case()["scores"]["visible"].tolist()
    assert sizes.min() > 6 and len(set(sizes.tolist())) == 8
    idx = seam_index(P, 8)
    assert_seam_visible(res, idx)
    assert_seam_visible(sizes, idx)
    pyr = S.pyramid_ref_records(kind, S.PYR2, small=small)
    assert np.array_equal(pyr[2][1], sizes) and pyr[2][0].min() > 6 and (pyr[2][0] < pyr[2][1]).all()
    assert_seam_visible(S.pyramid_rows(pyr), idx)
    for l in range(2):
        assert_seam_visible(pyr[1][l], idx)
        assert_seam_visible(pyr[2][l], idx)
    if not small:                                                   # the row scan's seam: four levels
        pyr4 = S.pyramid_ref_records(kind, S.PYR4)
        sidx = seam_index(S.SCAN_P, 8, S.SCAN_SEAM)
        assert (pyr4[2] > 0).all() and np.array_equal(pyr4[2][3], sizes)
        assert_seam_visible(S.pyramid_rows(pyr4), sidx, S.SCAN_SEAM)
        assert_seam_visible(pyr4[2][3], sidx, S.SCAN_SEAM)            # the seam lies in the last level: its cloud sizes ...
        if kind == "nn":                                             # ... and records (on the projective scene four poses lose every inlier on the way
            assert_seam_visible(pyr4[1][3], sidx, S.SCAN_SEAM)        # down and end with the untouched record; their sizes and final transforms differ)
        # a scan piece without its offset reads image j = (level 0, hypothesis j) for image 32768 + j = (level 3, hypothesis 8168 + j)
        assert (pyr4[2][3][sidx[S.SCAN_SEAM:]] != pyr4[2][0][sidx[:S.SCAN_P - S.SCAN_SEAM]]).all()


def test_clouds_and_mixed_rows_differ_across_the_seam():
    """The information tests' inputs (clouds, centres, radii through the index) and the mixed batches' (mesh, pose) pairs."""
    clouds = S.split_clouds()
    assert [len(x) for x in clouds] == [301, 394, 272, 176, 172, 123, 161, 670]
    idx = seam_index(P, 8)
    assert_seam_visible(np.array([[len(x)] + x[:100].reshape(-1).tolist() for x in clouds], np.float32), idx)
    m = S.mesh_runs(P)
    pair = np.stack([m, idx.astype(np.uint32)], 1)                   # (mesh, pose) of every hypothesis: 16 pairs, each before the seam
    assert len({tuple(r) for r in pair[:SEAM].tolist()}) == 16 and (pair[SEAM:, 1] != pair[:5, 1]).all()
