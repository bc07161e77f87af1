"""The size rule of a depth frame (csrc/frame_stage.h: depth_frame_ok -- 1 .. 65535 on a side, at most 2^26 pixels) at every entry point under
it: each refuses the same sizes with PR_ERR_INVALID and leaves its outputs untouched.  The device forms refuse before they touch a device, and
nothing is read before the refusal (the buffers hold 4 pixels), so all of this runs without a GPU.  The per-stage refusal tables (parameters,
null pointers, ...) are in the stages' own test files."""
import ctypes as C

import numpy as np
import pytest

from pose_refine_amd import _lib, api

BAD_FRAMES = [(0, 7), (7, 0), (65536, 1), (1, 65536), (65535, 1025), (8193, 8192)]
BAD_COUNTS = [0, 2 ** 26 + 1]
FX = (500.0, 500.0, 1.0, 1.0)


class Outputs:
    """Output buffers of 4 pixels prefilled with a sentinel."""

    def __init__(self):
        self.made = []

    def new(self, dtype, n=4):
        a = np.frombuffer(b"\xEE" * (n * np.dtype(dtype).itemsize), dtype).copy()
        self.made.append((a, a.tobytes()))
        return _lib.ptr(a)

    def untouched(self):
        return all(a.tobytes() == before for a, before in self.made)


def source(width, height):
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    return _lib.ReprojectSourceDesc(_lib.ptr(DEPTH), 0, _lib.SRC_DEPTH_U16, width, height, 0, *FX, eye)


DEPTH = np.full(4, 1000, np.uint16)
LABELS = np.ones(4, np.uint16)
KEEP = np.ones(2, np.uint8)
SEGMENT = np.zeros(1, _lib.SEGMENT)                                  # the box [0, 0] x [0, 0]: inside every frame


def segments(fn):
    def call(lib, o, w, h):
        sp, n = api.SegmentParams(), C.c_uint32(0xEEEEEEEE)
        rc = getattr(lib, fn)(_lib.ptr(DEPTH), 0, w, h, C.addressof(sp), o.new(np.uint16), o.new(np.uint32), o.new(_lib.SEGMENT), C.byref(n), None, None)
        return rc, n.value == 0xEEEEEEEE
    return call


def segment_roi(lib, o, w, h):
    roi = _lib.Roi(-7, -7, -7, -7)
    rc = lib.pr_segment_roi(_lib.ptr(SEGMENT), w, h, 0, C.byref(roi))
    return rc, (roi.x, roi.y, roi.width, roi.height) == (-7, -7, -7, -7)


def depth_filter(fn):
    def call(lib, o, w, h):
        dp, cnt = api.DepthFilterParams(), _lib.DepthFilterCounts()
        C.memset(C.addressof(cnt), 0x5A, C.sizeof(cnt))
        rc = getattr(lib, fn)(_lib.ptr(DEPTH), 0, w, h, C.addressof(dp), o.new(np.uint16), o.new(np.uint8), C.addressof(cnt))
        return rc, bytes(cnt) == b"\x5a" * C.sizeof(cnt)
    return call


def reproject(fn, bad_source):
    def call(lib, o, w, h):
        rp, cnt = api.ReprojectParams(), _lib.ReprojectCounts()
        C.memset(C.addressof(cnt), 0x5A, C.sizeof(cnt))
        table = (_lib.ReprojectSourceDesc * 1)(source(w, h) if bad_source else source(2, 2))
        tw, th = (2, 2) if bad_source else (w, h)
        rc = getattr(lib, fn)(C.addressof(table), 1, tw, th, *FX, 0, C.addressof(rp), o.new(np.uint16), o.new(np.uint8), C.addressof(cnt))
        return rc, bytes(cnt) == b"\x5a" * C.sizeof(cnt)
    return call


def depth_fuse(fn):
    def call(lib, o, n_px):
        table = (C.c_void_p * 1)(_lib.ptr(DEPTH))
        return getattr(lib, fn)(C.addressof(table), 1, 0, n_px, 1, o.new(np.uint16), o.new(np.uint8)), True
    return call


def segment_depth(lib, o, n_px):
    return lib.pr_segment_depth_dev(_lib.ptr(LABELS), _lib.ptr(DEPTH), 0, n_px, _lib.ptr(KEEP), len(KEEP), o.new(np.uint16)), True


ENTRY_POINTS = [
    ("pr_scene_segments_host", segments("pr_scene_segments_host"), BAD_FRAMES), ("pr_scene_segments_dev", segments("pr_scene_segments_dev"), BAD_FRAMES),
    ("pr_segment_roi", segment_roi, BAD_FRAMES),
    ("pr_depth_filter_host", depth_filter("pr_depth_filter_host"), BAD_FRAMES), ("pr_depth_filter_dev", depth_filter("pr_depth_filter_dev"), BAD_FRAMES),
    ("pr_depth_reproject_host-target", reproject("pr_depth_reproject_host", False), BAD_FRAMES),
    ("pr_depth_reproject_host-source", reproject("pr_depth_reproject_host", True), BAD_FRAMES),
    ("pr_depth_reproject_dev-target", reproject("pr_depth_reproject_dev", False), BAD_FRAMES),
    ("pr_depth_reproject_dev-source", reproject("pr_depth_reproject_dev", True), BAD_FRAMES),
    ("pr_depth_fuse_host", depth_fuse("pr_depth_fuse_host"), [(n,) for n in BAD_COUNTS]), ("pr_depth_fuse_dev", depth_fuse("pr_depth_fuse_dev"), [(n,) for n in BAD_COUNTS]),
    ("pr_segment_depth_dev", segment_depth, [(n,) for n in BAD_COUNTS]),
]


@pytest.mark.parametrize("name,call,sizes", ENTRY_POINTS, ids=[e[0] for e in ENTRY_POINTS])
def test_every_entry_point_refuses_the_same_frame_sizes(name, call, sizes):
    lib = _lib.load()
    for size in sizes:
        o = Outputs()
        rc, rest_untouched = call(lib, o, *size)
        assert rc == _lib.PR_ERR_INVALID, (name, size)
        assert o.untouched() and rest_untouched, (name, size)
        said = lib.pr_last_error().decode()
        assert name.split("-")[0] in said and str(size[0]) in said, (name, size, said)      # the refusal names its entry point and the offending value


def test_a_side_may_be_longer_than_8192():
    """65535 x 1: the side limit of a depth frame is not the renderer's 8192 (frame_ok, which the stages that take a scene keep)."""
    depth = np.full((1, 65535), 1000, np.uint16)
    depth[0, ::1000] = 0
    segs, labels, counts = api.scene_segments_host(depth, 65535, 1, min_pixels=1)
    assert counts[0] == len(segs) == 64 and (labels != 0).sum() == (depth != 0).sum()      # 66 runs of 999 pixels, the 64 largest labelled, the rest dropped
    out, counts = api.depth_filter_host(depth, 65535, 1)
    assert out.tobytes() == depth.tobytes() and sum(counts) == 65535
