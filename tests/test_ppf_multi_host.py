"""pr_ppf_vote_multi, the parts that need no device: the layout of pr_ppf_model, the calls that have nothing to do, and every refusal of the
header -- all of which come before any device is touched (a fake non-null device pointer is never dereferenced)."""
import ctypes as C
import os

import numpy as np
import pytest

from pose_refine_amd import _lib, api

FAKE = 0x10000                                                      # a non-null "device pointer"
HOST = np.zeros((4, 3), np.float32)                                 # a real host array for the sample pointers (never read either: the checks come first)


def _desc(pp, **kw):
    a = dict(params=C.addressof(pp), offsets_dev=FAKE, entries_dev=FAKE, points_host=_lib.ptr(HOST), normals_host=_lib.ptr(HOST), n_model=100, reserved=0)
    a.update(kw)
    return _lib.PPFModelDesc(**a)


def _vote(descs, n_models=None, **kw):
    """pr_ppf_vote_multi on a table of descriptors; the outputs are filled with 0xAB: (rc, outputs untouched)."""
    a = dict(sp=FAKE, sn=FAKE, n_scene=500, ref_first=0, ref_stride=1, n_refs=8, n_peaks=1)
    a.update(kw)
    table = (_lib.PPFModelDesc * max(1, len(descs)))(*descs)
    n_out = max(1, len(descs)) * 8 * 4                              # room for what a call with 8 references and 4 peaks would write
    peaks, poses = np.full(n_out * 16, 0xAB, np.uint8), np.full(n_out * 64, 0xAB, np.uint8)
    before = peaks.tobytes(), poses.tobytes()
    rc = _lib.load().pr_ppf_vote_multi(C.addressof(table), len(descs) if n_models is None else n_models, a["sp"], a["sn"], a["n_scene"], a["ref_first"],
                                       a["ref_stride"], a["n_refs"], a["n_peaks"], a.get("peaks", _lib.ptr(peaks)), a.get("poses", _lib.ptr(poses)), None)
    return rc, (peaks.tobytes(), poses.tobytes()) == before


def test_model_record_layout():
    assert C.sizeof(_lib.PPFModelDesc) == 48 and _lib.PPF_MAX_MODELS == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pose_refine.h")).read()
    assert "#define PR_PPF_MAX_MODELS 32" in header


def test_nothing_to_do_needs_no_device():
    pp = api.ppf_describe(100.0, 5.0, 15, 30)
    assert _vote([], n_models=0) == (_lib.PR_OK, True)
    assert _vote([_desc(pp), _desc(pp)], n_refs=0) == (_lib.PR_OK, True)
    assert _vote([_desc(pp)], n_refs=0, peaks=None, poses=None)[0] == _lib.PR_OK


def test_refusals_come_before_the_device():
    lib = _lib.load()
    pp = api.ppf_describe(100.0, 5.0, 15, 30)
    good = lambda: _desc(pp)
    assert _vote([good()] * 33) == (_lib.PR_ERR_INVALID, True)                                  # PR_PPF_MAX_MODELS = 32
    assert "PR_PPF_MAX_MODELS" in lib.pr_last_error().decode()
    odd = api.ppf_describe(100.0, 5.0, 15, 30)
    odd.n_alpha = 29
    assert _vote([good(), good(), _desc(odd)]) == (_lib.PR_ERR_INVALID, True)                   # a bad descriptor at index 2 of 3
    assert "model 2" in lib.pr_last_error().decode() and "n_alpha" in lib.pr_last_error().decode()
    assert _vote([good(), _desc(pp, reserved=1)]) == (_lib.PR_ERR_INVALID, True)
    assert "model 1" in lib.pr_last_error().decode() and "reserved" in lib.pr_last_error().decode()
    assert _vote([good(), _desc(pp, n_model=1093)]) == (_lib.PR_ERR_INVALID, True)              # 1093 x 30 = 32790 cells > PR_PPF_MAX_CELLS
    assert "model 1" in lib.pr_last_error().decode() and "PR_PPF_MAX_CELLS" in lib.pr_last_error().decode()
    for kw in (dict(n_model=0), dict(n_model=2049), dict(params=None)):
        assert _vote([_desc(pp, **kw), good()]) == (_lib.PR_ERR_INVALID, True), kw
        assert "model 0" in lib.pr_last_error().decode()
    for kw in (dict(points_host=None), dict(normals_host=None), dict(offsets_dev=None), dict(entries_dev=None)):       # a null sample or table pointer
        assert _vote([good(), _desc(pp, **kw)]) == (_lib.PR_ERR_INVALID, True), kw
        assert "model 1" in lib.pr_last_error().decode()
    assert _vote([good()], ref_first=493, n_refs=8) == (_lib.PR_ERR_INVALID, True)              # the reference window beyond n_scene
    assert _vote([good()], ref_stride=100, n_refs=6) == (_lib.PR_ERR_INVALID, True)
    assert _vote([good()], n_peaks=5) == (_lib.PR_ERR_INVALID, True)
    for kw in (dict(n_peaks=0), dict(ref_stride=0), dict(n_scene=0), dict(n_scene=16385), dict(ref_first=500), dict(sp=None), dict(sn=None),
               dict(peaks=None), dict(poses=None)):
        assert _vote([good()], **kw) == (_lib.PR_ERR_INVALID, True), kw
    assert lib.pr_ppf_vote_multi(None, 1, FAKE, FAKE, 500, 0, 1, 8, 1, FAKE, FAKE, None) == _lib.PR_ERR_INVALID       # a null table


def test_generate_hypotheses_multi_rejects_an_empty_list():
    with pytest.raises(ValueError):
        api.generate_hypotheses_multi([], None)
    with pytest.raises(ValueError):
        api.ppf_vote_multi([None] * 33, None, None, 500)
