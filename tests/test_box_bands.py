"""The banded layout of a depth box (asynchronous path, option box_bands) through its host twin, pr_debug_box_layout: pose_box.h -- the source the
kernels that fill, raster, count and emit a box address it with -- compiled for the host, no device.  Every pixel of a box must have its own
int below the slot's size, a tight box must never need more than the loose box that sized the batch, a sub-batch must fit the workspace
bound, and on the benchmark's hypotheses the layout must really cut the raster's 64-byte atomic requests."""
import os
import sys

import numpy as np
import pytest

from pose_refine_amd import api, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import raster_atomic_shape as shape  # noqa: E402

W, H = synth.WIDTH, synth.HEIGHT


def pixels(box):
    """(xs, image rows) of every pixel of the box {x0, y0, x1, y1} (raster y) -- the frame height comes with the caller's box."""
    xs, ys = np.meshgrid(np.arange(box[0], box[2] + 1), np.arange(box[1], box[3] + 1))
    return xs.ravel(), ys.ravel()


def check_box(box, w, h):
    """Offsets of the box's pixels: distinct, below the slot's size; the slot rounded as the packed layout rounds; the formula itself."""
    xs, ys = pixels(box)
    rows = h - 1 - ys
    pack = api.get_option("box_pack")
    for bands in (True, False):
        slot, off = api.box_layout(box, w, h, bands, xs, rows)
        assert slot % pack == 0
        assert len(np.unique(off)) == len(off), (box, w, h, bands)
        assert int(off.max()) < slot, (box, w, h, bands)
        bw = box[2] - box[0] + 1
        if bands:
            r0, r1 = h - 1 - box[3], h - 1 - box[1]
            R = r0 & ~3
            nb = ((r1 | 3) - R + 1) // 4
            assert slot == (4 * bw * nb + pack - 1) // pack * pack
            assert np.array_equal(off, (((rows >> 2) - (R >> 2)) * bw + (xs - box[0])) * 4 + (rows & 3))
        else:
            assert slot == (bw * (box[3] - box[1] + 1) + pack - 1) // pack * pack
    return api.box_layout(box, w, h, True)[0]


def test_every_width_and_every_row_alignment():
    """Widths 1..40 and every (r0 mod 4, r1 mod 4): one band, and several."""
    h = 64
    for bw in range(1, 41):
        for a in range(4):                                          # r0 = 8 + a
            for b in range(4):
                for r1 in (8 + b, 20 + b):
                    r0 = 8 + a
                    if r1 < r0:
                        continue
                    check_box([3, h - 1 - r1, 3 + bw - 1, h - 1 - r0], 64, h)


@pytest.mark.parametrize("w,h", [(640, 480), (161, 123)])
def test_full_frame_box(w, h):
    slot = check_box([0, 0, w - 1, h - 1], w, h)
    assert slot <= w * ((h + 3) & ~3) + api.get_option("box_pack")


def test_empty_box_has_no_slot():
    for box in ([5, 5, 4, 9], [5, 9, 8, 5], [0, 0, -1, -1]):
        for bands in (True, False):
            assert api.box_layout(box, W, H, bands)[0] == 0


def test_pixel_outside_the_box_is_refused():
    with pytest.raises(Exception):
        api.box_layout([4, 4, 9, 9], W, H, True, [10], [H - 1 - 5])


def random_box(rng, x0, y0, x1, y1):
    ax, bx = np.sort(rng.integers(x0, x1 + 1, 2))
    ay, by = np.sort(rng.integers(y0, y1 + 1, 2))
    return [int(ax), int(ay), int(bx), int(by)]


@pytest.mark.parametrize("w,h", [(640, 480), (161, 123)])
def test_tight_slot_never_exceeds_the_loose_one(w, h):
    """What keeps every offset and capacity derived from the loose boxes valid once the device has replaced them by tight ones."""
    rng = np.random.default_rng(7)
    for _ in range(4000):
        loose = random_box(rng, 0, 0, w - 1, h - 1)
        tight = random_box(rng, *loose)
        for bands in (True, False):
            assert api.box_layout(tight, w, h, bands)[0] <= api.box_layout(loose, w, h, bands)[0], (tight, loose, bands)


@pytest.mark.parametrize("w,h", [(640, 480), (161, 123)])
def test_slots_of_a_sub_batch_fit_the_workspace(w, h):
    """sub x (W x ((H + 3) & ~3) + kBoxPack) ints: random boxes, and the worst case -- every box the whole frame."""
    rng = np.random.default_rng(11)
    pack = api.get_option("box_pack")
    sub = 64
    bound = sub * (w * ((h + 3) & ~3) + pack)
    boxes = [random_box(rng, 0, 0, w - 1, h - 1) for _ in range(sub)]
    assert sum(api.box_layout(b, w, h, True)[0] for b in boxes) <= bound
    assert sub * api.box_layout([0, 0, w - 1, h - 1], w, h, True)[0] <= bound


def test_bands_cut_the_atomic_requests_of_the_benchmark_hypotheses():
    """The first 6 benchmark hypotheses, mesh in shipped order: at most 0.75 of the row-major requests (counted: 0.65; the cap leaves room
    for a different patch shape and none for no effect)."""
    tris = shape.shipped_order(shape.load_obj06())
    poses = synth.hypotheses(6)
    rows = shape.requests_per_hypothesis(tris, poses)
    bands = shape.requests_per_hypothesis(tris, poses, "bands")
    print(f"64-B requests per hypothesis: row-major {rows:.0f}, banded {bands:.0f}, ratio {bands / rows:.3f}")
    assert bands <= 0.75 * rows
