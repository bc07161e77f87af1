"""Depth conditioning on the device: pr_depth_filter_dev and pr_depth_fuse_dev against the numpy reference (tests/depth_filter_ref.py) and the
host twins byte for byte -- depth, flags, counts --, the same call twice, the optional outputs left out, refusals that leave the device buffers
untouched, and the hand-over of a cleaned 640 x 480 frame to the stages behind it.  Bytes and hand-over only: no accuracy figure is asserted here
(tests/test_depth_filter_host.py holds the definition to what it is for)."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_cases as DC
import depth_filter_ref as R
from pose_refine_amd import _lib, api

pytestmark = pytest.mark.gpu

FILTER_CASES = DC.filter_cases()
FUSE_CASES = DC.fuse_cases()


def run_dev(d, params, want_flags=True):
    h, w = d.shape
    res = api.depth_filter(d, w, h, want_flags=want_flags, **params)
    return tuple(r.to_host().reshape(h, w) if isinstance(r, api.DeviceVector) else r for r in res)


@pytest.mark.parametrize("case", FILTER_CASES, ids=[c[0] for c in FILTER_CASES])
def test_filter_device_equals_reference_and_host(gpu, case):
    name, depth, params = case
    h, w = depth.shape
    for dtype in DC.dtypes_of(depth):
        what = f"{name} {np.dtype(dtype).name}"
        d = depth.astype(dtype)
        ref = R.depth_filter(d, params)
        got = run_dev(d, params)
        assert got[0].dtype == dtype and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2], what
        host = api.depth_filter_host(d, w, h, want_flags=True, **params)
        assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes() and got[2] == host[2], what
        again = run_dev(d, params)                                              # the same call twice
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2], what
        bare = run_dev(d, params, want_flags=False)                             # flags_dev_out NULL
        assert bare[0].tobytes() == got[0].tobytes() and bare[1] == got[2], what


def test_filter_null_flags_and_counts(gpu):
    _, depth, params = next(c for c in FILTER_CASES if c[0] == "130x77_all_r2")
    h, w = depth.shape
    for dtype in (np.uint16, np.int32):
        d = depth.astype(dtype)
        src, out = api.DeviceVector.from_host(d.reshape(-1)), api.DeviceVector(w * h, dtype)
        dp = api.DepthFilterParams(**params)
        _lib.check(_lib.load().pr_depth_filter_dev(src.data(), int(dtype == np.int32), w, h, C.addressof(dp), out.data(), None, None))
        assert out.to_host().tobytes() == R.depth_filter(d, params)[0].tobytes()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_filter_refusals_leave_the_device_buffers(gpu, dtype):
    lib = _lib.load()
    _, depth, params = next(c for c in FILTER_CASES if c[0] == "67x45_all_r1")
    h, w = depth.shape
    d = depth.astype(dtype)
    src = api.DeviceVector.from_host(d.reshape(-1))
    out = api.DeviceVector.from_host(np.full(w * h, 0x2BCD, dtype))
    flags = api.DeviceVector.from_host(np.full(w * h, 0xEE, np.uint8))
    good = api.DepthFilterParams(**params)
    bad = _lib.DepthFilterParamsDesc.from_buffer_copy(bytes(good))
    bad.radius = 3
    cnt = _lib.DepthFilterCounts()
    C.memset(C.addressof(cnt), 0x5A, 32)
    i32 = int(dtype == np.int32)
    assert lib.pr_depth_filter_dev(src.data(), i32, w, h, C.addressof(good), src.data(), flags.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID      # out == in
    assert lib.pr_depth_filter_dev(src.data(), i32, w, h, C.addressof(bad), out.data(), flags.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert lib.pr_depth_filter_dev(src.data(), i32, w, 0, C.addressof(good), out.data(), flags.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert src.to_host().tobytes() == d.tobytes() and (out.to_host() == 0x2BCD).all() and (flags.to_host() == 0xEE).all() and bytes(cnt) == b"\x5a" * 32
    # the next call on the same context is not disturbed
    ref = R.depth_filter(d, params)
    got = run_dev(d, params)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]


# ---- the fuse ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FUSE_CASES, ids=[c[0] for c in FUSE_CASES])
def test_fuse_device_equals_reference_and_host(gpu, case):
    name, frames, min_frames = case
    n_px = frames.shape[1]
    for dtype in DC.dtypes_of(frames):
        what = f"{name} {np.dtype(dtype).name}"
        fs = [f.astype(dtype) for f in frames]
        ref_out, ref_count = R.depth_fuse(fs, min_frames)
        dev = [api.DeviceVector.from_host(f) for f in fs]
        out, count = api.depth_fuse(dev, n_px, 1, min_frames=min_frames, want_count=True)
        assert out.dtype == dtype and out.to_host().tobytes() == ref_out.tobytes() and count.to_host().tobytes() == ref_count.tobytes(), what
        host = api.depth_fuse_host(fs, n_px, 1, min_frames=min_frames)
        assert out.to_host().tobytes() == host.tobytes(), what
        again = api.depth_fuse(dev, n_px, 1, min_frames=min_frames)             # the same call twice; count_out NULL
        assert again.to_host().tobytes() == ref_out.tobytes(), what


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("n_px", [203, 1031])
def test_fuse_repeated_pointer_in_place_and_offset(gpu, dtype, n_px):
    lib = _lib.load()
    frames = [f.astype(dtype) for f in DC.fuse_frames(3, n_px + 1, seed=n_px)]
    a, b, c = [api.DeviceVector.from_host(f) for f in frames]
    i32 = int(dtype == np.int32)
    # the same pointer three times, depth_out one of the frames
    ref_out, ref_count = R.depth_fuse([frames[0], frames[1], frames[0], frames[2], frames[0]], 2)
    out, count = api.depth_fuse([a, b, a, c, a], n_px + 1, 1, min_frames=2, depth_out=b, want_count=True)
    assert out is b and b.to_host().tobytes() == ref_out.tobytes() and count.to_host().tobytes() == ref_count.tobytes()
    # base pointers one element in: off the 16-byte bound, the lane-per-pixel path; the element in front of the output stays
    step = np.dtype(dtype).itemsize
    a2, c2 = api.DeviceVector.from_host(frames[0]), api.DeviceVector.from_host(frames[2])
    dst = api.DeviceVector.from_host(np.full(n_px + 1, 0x2BCD, dtype))
    cnt = api.DeviceVector.from_host(np.full(n_px + 1, 0xEE, np.uint8))
    table = (C.c_void_p * 2)(a2.data() + step, c2.data() + step)
    _lib.check(lib.pr_depth_fuse_dev(C.addressof(table), 2, i32, n_px, 1, dst.data() + step, cnt.data() + 1))
    ref_out, ref_count = R.depth_fuse([frames[0][1:], frames[2][1:]], 1)
    got, got_count = dst.to_host(), cnt.to_host()
    assert got[0] == 0x2BCD and got[1:].tobytes() == ref_out.tobytes() and got_count[0] == 0xEE and got_count[1:].tobytes() == ref_count.tobytes()
    # aligned frames and output, the counts one byte in: the counts decide the path as well
    cnt2 = api.DeviceVector.from_host(np.full(n_px + 2, 0xEE, np.uint8))
    table = (C.c_void_p * 2)(a2.data(), c2.data())
    _lib.check(lib.pr_depth_fuse_dev(C.addressof(table), 2, i32, n_px + 1, 2, dst.data(), cnt2.data() + 1))
    ref_out, ref_count = R.depth_fuse([frames[0], frames[2]], 2)
    assert dst.to_host().tobytes() == ref_out.tobytes() and cnt2.to_host()[1:].tobytes() == ref_count.tobytes() and cnt2.to_host()[0] == 0xEE


def test_fuse_refusal_leaves_the_device_buffers(gpu):
    lib = _lib.load()
    a = api.DeviceVector.from_host(np.full(100, 7, np.uint16))
    out = api.DeviceVector.from_host(np.full(100, 0x2BCD, np.uint16))
    table = (C.c_void_p * 2)(a.data(), a.data())
    assert lib.pr_depth_fuse_dev(C.addressof(table), 2, 0, 100, 3, out.data(), None) == _lib.PR_ERR_INVALID
    assert (out.to_host() == 0x2BCD).all()
    assert (api.depth_fuse([a, a], 100, 1, min_frames=2).to_host() == 7).all()


# ---- the hand-over at the workload's size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_hand_over_at_640x480(gpu, dtype):
    W, H, f = 640, 480, 600.0
    clean = R.clean_scene(W, H, f)
    frame = R.corrupt(clean, 0, hole_block=((160, 163), (200, 203)))[0].astype(dtype)
    params = dict(min_mm=100, max_mm=2000, tol_mm=8, tol_permille=5, fly_min_support=3, radius=2, fill_min=13)
    src = api.DeviceVector.from_host(frame.reshape(-1))
    out, flags, counts = api.depth_filter(src, W, H, want_flags=True, **params)
    host = api.depth_filter_host(frame, W, H, want_flags=True, **params)
    assert out.dtype == dtype and out.size() == W * H
    assert out.to_host().tobytes() == host[0].tobytes() and flags.to_host().tobytes() == host[1].tobytes() and counts == host[2]
    assert src.to_host().tobytes() == frame.tobytes()                            # the input is left as it was
    # the cleaned DeviceVector goes as it is into the stages behind it
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    scene = api.Scene_projective().init_Scene_projective_device(out, K, W, H)
    planes, labels, cleared = api.scene_planes(scene, out)
    assert labels.size() == W * H and cleared.dtype == dtype and cleared.size() == W * H
    segs, seg_labels, seg_counts = api.scene_segments(out, W, H, jump_mm=20)
    host_segs = api.scene_segments_host(host[0], W, H, jump_mm=20)
    assert seg_labels.size() == W * H and seg_counts == host_segs[-1] and segs.tobytes() == host_segs[0].tobytes()
