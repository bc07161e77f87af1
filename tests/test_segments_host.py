"""Scene segments on the host: pr_scene_segments_host against the numpy reference (tests/segments_ref.py) byte for byte -- labels, roots, records
and the three counts -- the reference against a second formulation, every refusal, and pr_segment_roi.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import segments_cases as SC
import segments_ref as R
from pose_refine_amd import _lib, api


def run_host(depth, dtype, kw):
    segs, labels, roots, counts = api.scene_segments_host(depth.astype(dtype), depth.shape[1], depth.shape[0], want_roots=True, **kw)
    return segs, labels, roots, counts


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_equals_reference(name):
    c, ref = SC.BY_NAME[name], SC.reference(name)
    for dtype in c.dtypes:
        SC.assert_same(run_host(c.depth, dtype, c.kw), ref, f"{name} {np.dtype(dtype).name}")


@pytest.mark.parametrize("name", SC.SMALL)
def test_reference_equals_minimum_propagation(name):
    c, ref = SC.BY_NAME[name], SC.reference(name)
    assert np.array_equal(R.roots_by_min_propagation(c.depth, c.kw["jump_mm"]), ref["roots"])


def test_the_cases_are_what_they_are_meant_to_be():
    for w, h in SC.SIZES:
        tag = f"{w}x{h}"
        sp = SC.reference(f"spiral_{tag}")
        assert sp["counts"] == (1, 1, 1) and sp["segments"][0]["pixels"] > 0.4 * w * h               # one path, about half the frame long
        two = SC.reference(f"spirals_interleaved_{tag}")
        assert two["counts"][2] == 2 and not (two["labels"] == 0).any()
        assert SC.reference(f"noise_{tag}")["counts"][2] > 0.05 * w * h                                # thousands of components at the largest size
    assert SC.reference("noise_200x150")["counts"][2] > 2000
    for tag in ("67x45", "130x77"):
        w = int(tag.split("x")[0])
        assert SC.reference(f"comb_{tag}")["counts"] == (1, 1, 1) and SC.reference(f"u_shapes_{tag}")["counts"] == (1, 1, 1)
        assert SC.reference(f"combs_interlocked_{tag}")["counts"] == (2, 2, 2)
        one = SC.reference(f"staircase_{tag}")
        assert one["counts"] == (1, 1, 1) and one["segments"][0]["depth_max"] - one["segments"][0]["depth_min"] == SC.JUMP * (w - 1)
        assert SC.reference(f"staircase_cut_{tag}")["counts"] == (2, 2, 2)
        few = SC.reference(f"noise_few_{tag}")
        assert few["counts"][0] == 5 < few["counts"][1] < few["counts"][2] and (few["labels"] == R.SEGMENT_DROPPED).any()
        assert SC.reference(f"empty_{tag}")["counts"] == (0, 0, 0) and not SC.reference(f"empty_{tag}")["labels"].any()
    # ties: four squares of 100 pixels in root order, then the two of 64, then the one of 36
    sq = SC.reference("squares_min1")["segments"]
    assert list(sq["pixels"]) == [100, 100, 100, 100, 64, 64, 36] and (np.diff(sq["root"][:4].astype(np.int64)) > 0).all() and sq["root"][4] < sq["root"][5]
    assert [SC.reference(f"squares_min{m}")["counts"][1] for m in (64, 65, 100, 101)] == [6, 4, 4, 0]
    assert SC.reference("squares_max3")["counts"][:2] == (3, 7)
    const = SC.reference("constant_640x480")
    assert const["counts"] == (1, 1, 1) and const["segments"][0]["sum_depth"] == 65535 * 640 * 480
    lo, hi = SC.reference(f"int32_extremes_jump{SC.JUMP}"), SC.reference(f"int32_extremes_jump{SC.I32_MAX}")
    ext = SC.BY_NAME[f"int32_extremes_jump{SC.JUMP}"].depth
    assert (lo["labels"][ext <= 0] == 0).all() and (lo["labels"][ext > 0] != 0).all()
    assert lo["roots"][10, 10] != lo["roots"][10, 11] and hi["roots"][10, 10] == hi["roots"][10, 11]        # 1 next to 2^31 - 1
    assert SC.reference(f"int32_extremes_jump{SC.I32_MAX - 2}")["roots"][10, 10] == hi["roots"][10, 10] and lo["counts"][2] > hi["counts"][2]


def test_root_cap_refuses_and_writes_nothing():
    d = SC.CHECKERBOARD
    with pytest.raises(R.Refused):
        R.scene_segments(d, **SC.CHECKERBOARD_KW)
    h, w = d.shape
    for dtype in (np.uint16, np.int32):
        dep = d.astype(dtype)
        sp = api.SegmentParams(**SC.CHECKERBOARD_KW)
        labels, roots = np.full((h, w), 0xABCD, np.uint16), np.full((h, w), 0x12345678, np.uint32)
        segs = np.full(sp.max_segments, 0x5A, np.uint8).repeat(64).view(_lib.SEGMENT)
        n = [C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)]
        rc = _lib.load().pr_scene_segments_host(_lib.ptr(dep), int(dtype == np.int32), w, h, C.addressof(sp), _lib.ptr(labels), _lib.ptr(roots), _lib.ptr(segs),
                                                *[C.byref(v) for v in n])
        assert rc == _lib.PR_ERR_INVALID
        assert (labels == 0xABCD).all() and (roots == 0x12345678).all() and (segs.view(np.uint8) == 0x5A).all() and [v.value for v in n] == [77, 77, 77]
    # one more pixel per component allowed: exactly PR_SEGMENT_MAX_ROOTS is fine
    rows = R.SEGMENT_MAX_ROOTS // 185
    ok = d[:rows + 1, :].copy()
    ok.reshape(-1)[R.SEGMENT_MAX_ROOTS:] = 0
    segs, labels, counts = api.scene_segments_host(ok.astype(np.uint16), ok.shape[1], ok.shape[0], **SC.CHECKERBOARD_KW)
    assert counts == (64, R.SEGMENT_MAX_ROOTS, R.SEGMENT_MAX_ROOTS)


@pytest.mark.parametrize("args", [(10, 0, 64), (10, 1, 0), (10, 1, R.SEGMENT_MAX + 1), (2 ** 31, 1, 1)])
def test_describe_refuses(args):
    sp = _lib.SegmentParamsDesc(1, 2, 3, 4)
    assert _lib.load().pr_segment_describe(*args, C.addressof(sp)) == _lib.PR_ERR_INVALID
    assert (sp.jump_mm, sp.min_pixels, sp.max_segments, sp.reserved) == (1, 2, 3, 4)
    with pytest.raises(R.Refused):
        R.check_params(*args)


def test_describe_fills_and_null_out():
    assert _lib.load().pr_segment_describe(10, 1, 1, None) == _lib.PR_ERR_INVALID
    for args in [(0, 1, 1), (2 ** 31 - 1, 2 ** 32 - 1, R.SEGMENT_MAX)]:
        sp = api.SegmentParams(*args)
        assert (sp.jump_mm, sp.min_pixels, sp.max_segments, sp.reserved) == args + (0,)
        R.check_params(*args)
    sp = api.SegmentParams()
    assert (sp.jump_mm, sp.min_pixels, sp.max_segments) == (10, 256, 64)


@pytest.mark.parametrize("w,h", [(0, 5), (5, 0), (65536, 1), (1, 65536), (8193, 8192), (65535, 1025)])
def test_frame_size_refusals(w, h):
    with pytest.raises(R.Refused):
        R.check_frame(w, h)
    sp = api.SegmentParams(min_pixels=1)
    one = np.zeros(1, np.uint16)                                   # the size is refused before a pixel is read
    lab, seg, n = np.zeros(1, np.uint16), np.zeros(sp.max_segments, _lib.SEGMENT), C.c_uint32(0)
    assert _lib.load().pr_scene_segments_host(_lib.ptr(one), 0, w, h, C.addressof(sp), _lib.ptr(lab), None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
    assert _lib.load().pr_scene_segments_dev(_lib.ptr(one), 0, w, h, C.addressof(sp), _lib.ptr(lab), None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
    assert _lib.load().pr_segment_roi(_lib.ptr(seg), w, h, 0, C.byref(_lib.Roi())) == _lib.PR_ERR_INVALID


def test_largest_frames_are_accepted_by_the_size_check():
    R.check_frame(65535, 1024)
    R.check_frame(8192, 8192)
    seg = np.zeros(1, _lib.SEGMENT)
    for w, h in [(65535, 1024), (8192, 8192), (1, 65535)]:
        assert api.segment_roi(seg[0], w, h) == (0, 0, 1, 1)


def test_bad_parameter_blocks_and_null_pointers():
    d = np.ones((4, 4), np.uint16)
    lab, seg, n = np.zeros((4, 4), np.uint16), np.zeros(4, _lib.SEGMENT), C.c_uint32(0)
    lib = _lib.load()
    good = api.SegmentParams(min_pixels=1, max_segments=4)
    for bad in [_lib.SegmentParamsDesc(10, 0, 4, 0), _lib.SegmentParamsDesc(10, 1, 0, 0), _lib.SegmentParamsDesc(10, 1, 4097, 0), _lib.SegmentParamsDesc(2 ** 31, 1, 4, 0),
                _lib.SegmentParamsDesc(10, 1, 4, 1)]:
        for fn in (lib.pr_scene_segments_host, lib.pr_scene_segments_dev):
            assert fn(_lib.ptr(d), 0, 4, 4, C.addressof(bad), _lib.ptr(lab), None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
    for fn in (lib.pr_scene_segments_host, lib.pr_scene_segments_dev):   # checked before any device is touched: these answer without a GPU
        assert fn(_lib.ptr(d), 0, 4, 4, None, _lib.ptr(lab), None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
        assert fn(None, 0, 4, 4, C.addressof(good), _lib.ptr(lab), None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
        assert fn(_lib.ptr(d), 0, 4, 4, C.addressof(good), None, None, _lib.ptr(seg), C.byref(n), None, None) == _lib.PR_ERR_INVALID
        assert fn(_lib.ptr(d), 0, 4, 4, C.addressof(good), _lib.ptr(lab), None, None, C.byref(n), None, None) == _lib.PR_ERR_INVALID
        assert fn(_lib.ptr(d), 0, 4, 4, C.addressof(good), _lib.ptr(lab), None, _lib.ptr(seg), None, None, None) == _lib.PR_ERR_INVALID
    keep = np.ones(2, np.uint8)
    assert lib.pr_segment_depth_dev(None, _lib.ptr(d), 0, 16, _lib.ptr(keep), 2, _lib.ptr(d)) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_depth_dev(_lib.ptr(lab), _lib.ptr(d), 0, 0, _lib.ptr(keep), 2, _lib.ptr(d)) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_depth_dev(_lib.ptr(lab), _lib.ptr(d), 0, 2 ** 26 + 1, _lib.ptr(keep), 2, _lib.ptr(d)) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_depth_dev(_lib.ptr(lab), _lib.ptr(d), 0, 16, _lib.ptr(keep), R.SEGMENT_MAX + 2, _lib.ptr(d)) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_depth_dev(_lib.ptr(lab), _lib.ptr(d), 0, 16, None, 2, _lib.ptr(d)) == _lib.PR_ERR_INVALID
    # the optional outputs: NULL roots and counts give the same labels and records
    a = api.scene_segments_host(d, 4, 4, params=good)
    b = api.scene_segments_host(d, 4, 4, params=good, want_roots=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[-1] == b[-1] == (1, 1, 1)


def test_segment_roi_clips_at_all_four_borders():
    W, H = 67, 45
    seg = np.zeros(1, _lib.SEGMENT)[0]
    for box in [(0, 0, 3, 3), (60, 0, 66, 5), (0, 40, 4, 44), (63, 41, 66, 44), (20, 10, 30, 20), (0, 0, 66, 44)]:
        seg["x0"], seg["y0"], seg["x1"], seg["y1"] = box
        for margin in (0, 1, 5, 1000, 2 ** 32 - 1):
            roi = api.segment_roi(seg, W, H, margin)
            assert roi == R.segment_roi(seg, W, H, margin)
            assert roi[0] >= 0 and roi[1] >= 0 and roi[0] + roi[2] <= W and roi[1] + roi[3] <= H and roi[2] >= box[2] - box[0] + 1
        assert api.segment_roi(seg, W, H, 0) == (box[0], box[1], box[2] - box[0] + 1, box[3] - box[1] + 1)
    assert api.segment_roi(seg, W, H, 1000) == (0, 0, W, H)
    lib = _lib.load()
    rec = np.zeros(1, _lib.SEGMENT)
    for box in [(5, 5, 4, 9), (5, 5, 9, 4), (0, 0, 67, 3), (0, 0, 3, 45)]:          # an inverted box, a box outside the frame
        rec[0]["x0"], rec[0]["y0"], rec[0]["x1"], rec[0]["y1"] = box
        assert lib.pr_segment_roi(_lib.ptr(rec), W, H, 0, C.byref(_lib.Roi())) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_roi(None, W, H, 0, C.byref(_lib.Roi())) == _lib.PR_ERR_INVALID
    assert lib.pr_segment_roi(_lib.ptr(rec), W, H, 0, None) == _lib.PR_ERR_INVALID
