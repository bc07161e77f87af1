"""Depth conditioning on the host: pr_depth_filter_host and pr_depth_fuse_host against the numpy reference (tests/depth_filter_ref.py) byte for
byte -- depth, flags and counts --, every refusal with its outputs untouched, and the definition held to what it is for on an analytic scene
with injected noise, flying pixels and holes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_cases as DC
import depth_filter_ref as R
from pose_refine_amd import _lib, api

FILTER_CASES = DC.filter_cases()
FUSE_CASES = DC.fuse_cases()


@pytest.mark.parametrize("case", FILTER_CASES, ids=[c[0] for c in FILTER_CASES])
def test_filter_host_equals_reference(case):
    name, depth, params = case
    h, w = depth.shape
    for dtype in DC.dtypes_of(depth):
        d = depth.astype(dtype)
        ref_out, ref_flags, ref_counts = R.depth_filter(d, params)
        out, flags, counts = api.depth_filter_host(d, w, h, want_flags=True, **params)
        what = f"{name} {np.dtype(dtype).name}"
        assert out.dtype == dtype and out.tobytes() == ref_out.tobytes(), what
        assert flags.tobytes() == ref_flags.tobytes() and counts == ref_counts, what
        bare, bare_counts = api.depth_filter_host(d, w, h, **params)           # flags_out NULL
        assert bare.tobytes() == out.tobytes() and bare_counts == counts, what
        assert np.isin(out[out != 0], d).all(), what                            # every output value is an input value


def test_the_cases_are_what_they_are_meant_to_be():
    by_name = {c[0]: c for c in FILTER_CASES}

    def ref(name, dtype=np.int32):
        _, depth, params = by_name[name]
        return R.depth_filter(depth.astype(dtype), params)

    for tag in ("67x45", "130x77"):
        assert all(n > 0 for n in ref(f"{tag}_all_r1")[2]), tag                # every flag code occurs
        assert ref(f"{tag}_gate_all")[2][R.KEPT] == 0 and not ref(f"{tag}_gate_all")[0].any()
        assert ref(f"{tag}_median_r2_wide")[2][R.SMOOTHED] > 100
        assert ref(f"{tag}_fill_r2_min24")[2][R.FILLED] > 0 and ref(f"{tag}_fill_r1_min8")[2][R.FILLED] > 0
        assert ref(f"{tag}_fill_r1_min1")[2][R.UNMEASURED] > 0                 # the middle of the block of holes
        assert ref(f"{tag}_none")[0].tobytes() == by_name[f"{tag}_none"][1].astype(np.int32).tobytes()
    assert ref("even_3x3")[0][1, 1] == 1030
    assert ref("half_fill5")[0][1, 1] == 0 and ref("half_fill4")[0][1, 1] == 600
    assert ref("gated_in_ring")[1][2, 2] == R.GATED and ref("flying_in_ring")[1][2, 2] == R.FLYING and ref("flying_in_ring_r2")[0][2, 2] == 0
    assert ref("at_tol_support4")[1][1, 1] == R.KEPT and ref("at_tol_support5")[1][1, 1] == R.FLYING
    assert ref("at_tol_median")[0][1, 1] == 1000 and ref("i32_extremes_r2")[2][R.FILLED] > 0


@pytest.mark.parametrize("case", FUSE_CASES, ids=[c[0] for c in FUSE_CASES])
def test_fuse_host_equals_reference(case):
    name, frames, min_frames = case
    for dtype in DC.dtypes_of(frames):
        fs = [f.astype(dtype) for f in frames]
        ref_out, ref_count = R.depth_fuse(fs, min_frames)
        out, count = api.depth_fuse_host(fs, frames.shape[1], 1, min_frames=min_frames, want_count=True)
        what = f"{name} {np.dtype(dtype).name}"
        assert out.dtype == dtype and out.tobytes() == ref_out.tobytes() and count.tobytes() == ref_count.tobytes(), what
        assert api.depth_fuse_host(fs, frames.shape[1], 1, min_frames=min_frames).tobytes() == out.tobytes(), what      # count_out NULL


def test_fuse_host_repeated_pointer_and_in_place():
    frames = DC.fuse_frames(3, 203, seed=11).astype(np.uint16)
    a, b, c = [f.copy() for f in frames]
    ref_out, ref_count = R.depth_fuse([a, b, a, c, a], 2)                       # the same pointer three times
    table = (C.c_void_p * 5)(*[_lib.ptr(x) for x in (a, b, a, c, a)])
    count = np.zeros(203, np.uint8)
    _lib.check(_lib.load().pr_depth_fuse_host(C.addressof(table), 5, 0, 203, 2, _lib.ptr(b), _lib.ptr(count)))      # depth_out is frame 1
    assert b.tobytes() == ref_out.tobytes() and count.tobytes() == ref_count.tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
GOOD = dict(min_mm=100, max_mm=2000, tol_mm=8, tol_permille=5, fly_min_support=3, radius=1, fill_min=5)
BAD_PARAMS = [dict(min_mm=2 ** 31), dict(max_mm=2 ** 31), dict(tol_mm=2 ** 31), dict(min_mm=2001), dict(tol_permille=1001), dict(fly_min_support=9), dict(radius=3),
              dict(radius=0), dict(fill_min=9), dict(radius=2, fill_min=25), dict(radius=0, fill_min=0, reserved=1)]


def raw_params(**kw):
    p = _lib.DepthFilterParamsDesc()
    for k, v in dict(GOOD, **kw).items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=[str(b) for b in BAD_PARAMS])
def test_bad_parameters_are_refused(bad):
    lib = _lib.load()
    p = raw_params(**bad)
    if "reserved" not in bad:
        out = _lib.DepthFilterParamsDesc()
        C.memset(C.addressof(out), 0x5A, 32)
        rc = lib.pr_depth_filter_describe(p.min_mm, p.max_mm, p.tol_mm, p.tol_permille, p.fly_min_support, p.radius, p.fill_min, C.addressof(out))
        assert rc == _lib.PR_ERR_INVALID and bytes(out) == b"\x5a" * 32
    d = np.full((4, 5), 1000, np.uint16)
    out, flags, cnt = np.full((4, 5), 0xABCD, np.uint16), np.full((4, 5), 0xEE, np.uint8), _lib.DepthFilterCounts()
    C.memset(C.addressof(cnt), 0x5A, 32)
    assert lib.pr_depth_filter_host(_lib.ptr(d), 0, 5, 4, C.addressof(p), _lib.ptr(out), _lib.ptr(flags), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert (out == 0xABCD).all() and (flags == 0xEE).all() and bytes(cnt) == b"\x5a" * 32


def test_describe_accepts_the_limits():
    lim = api.DepthFilterParams(min_mm=2 ** 31 - 1, max_mm=2 ** 31 - 1, tol_mm=2 ** 31 - 1, tol_permille=1000, fly_min_support=8, radius=2, fill_min=24)
    assert (lim.min_mm, lim.fill_min, lim.reserved) == (2 ** 31 - 1, 24, 0)
    assert api.DepthFilterParams(min_mm=5000, max_mm=0).max_mm == 0              # no upper gate: min_mm may be anything
    off = api.DepthFilterParams()
    assert bytes(off) == b"\0" * 32                                             # no hidden default switches a stage on
    assert _lib.load().pr_depth_filter_describe(0, 0, 0, 0, 0, 0, 0, None) == _lib.PR_ERR_INVALID      # a null out


def test_filter_entry_point_refusals():
    lib, p = _lib.load(), raw_params()
    d = np.full((4, 5), 1000, np.uint16)
    out, flags = np.full((4, 5), 0xABCD, np.uint16), np.full((4, 5), 0xEE, np.uint8)
    calls = [
        (None, 5, 4, C.addressof(p), _lib.ptr(out)), (_lib.ptr(d), 5, 4, None, _lib.ptr(out)), (_lib.ptr(d), 5, 4, C.addressof(p), None),
        (_lib.ptr(out), 5, 4, C.addressof(p), _lib.ptr(out)),                   # depth_out == depth_in
        (_lib.ptr(d), 0, 4, C.addressof(p), _lib.ptr(out)), (_lib.ptr(d), 5, 0, C.addressof(p), _lib.ptr(out)),
        (_lib.ptr(d), 65536, 1, C.addressof(p), _lib.ptr(out)), (_lib.ptr(d), 1, 65536, C.addressof(p), _lib.ptr(out)),
        (_lib.ptr(d), 65535, 1025, C.addressof(p), _lib.ptr(out)),              # more than 2^26 pixels
    ]
    for fn in (lib.pr_depth_filter_host, lib.pr_depth_filter_dev):               # the device form refuses before it touches a device: this runs without one
        for i, (src, w, h, pp, dst) in enumerate(calls):
            assert fn(src, 0, w, h, pp, dst, _lib.ptr(flags), None) == _lib.PR_ERR_INVALID, i
            assert (out == 0xABCD).all() and (flags == 0xEE).all(), i


def test_fuse_entry_point_refusals():
    lib = _lib.load()
    a, out, count = np.full(10, 7, np.uint16), np.full(10, 0xABCD, np.uint16), np.full(10, 0xEE, np.uint8)
    one = (C.c_void_p * 9)(*[_lib.ptr(a)] * 9)
    hole = (C.c_void_p * 3)(_lib.ptr(a), None, _lib.ptr(a))
    calls = [(None, 1, 10, 1, _lib.ptr(out)), (C.addressof(one), 0, 10, 1, _lib.ptr(out)), (C.addressof(one), 9, 10, 1, _lib.ptr(out)),
             (C.addressof(one), 3, 10, 0, _lib.ptr(out)), (C.addressof(one), 3, 10, 4, _lib.ptr(out)), (C.addressof(one), 3, 0, 1, _lib.ptr(out)),
             (C.addressof(one), 3, 2 ** 26 + 1, 1, _lib.ptr(out)), (C.addressof(one), 3, 10, 1, None), (C.addressof(hole), 3, 10, 1, _lib.ptr(out))]
    for fn in (lib.pr_depth_fuse_host, lib.pr_depth_fuse_dev):
        for i, (tab, n, n_px, mf, dst) in enumerate(calls):
            assert fn(tab, n, 0, n_px, mf, dst, _lib.ptr(count)) == _lib.PR_ERR_INVALID, i
            assert (out == 0xABCD).all() and (count == 0xEE).all(), i


# ---- the property scenario: the definition held to what it is for ------------------------------------------------------------------------------
CLEAN = R.clean_scene()
SCENARIO = [dict(GOOD, radius=1, fill_min=5), dict(GOOD, radius=2, fill_min=13)]


def rms(a, b, where):
    return float(np.sqrt(np.mean((a[where].astype(np.float64) - b[where]) ** 2)))


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("params", SCENARIO, ids=["r1", "r2"])
def test_single_frame_properties(seed, params):
    frame, flying, holes = R.corrupt(CLEAN, seed)
    out, flags, counts = api.depth_filter_host(frame.astype(np.uint16), 160, 120, want_flags=True, **params)
    out = out.astype(np.int64)
    untouched = ~flying & ~holes
    removed = (flags[flying] == R.FLYING).mean()
    wrongly = (flags[untouched] == R.FLYING).mean()
    alive = untouched & (out != 0)
    before, after = rms(frame, CLEAN, alive), rms(out, CLEAN, alive)
    filled = flags == R.FILLED
    fill_err = np.abs(out - CLEAN)[filled]
    print(f"seed {seed} radius {params['radius']}: removed {removed:.4f} wrongly {wrongly:.4f} rms {before:.3f} -> {after:.3f} filled {filled.sum()} of {holes.sum()} "
          f"largest fill error {fill_err.max() if filled.any() else 0}")
    assert removed >= 0.95
    assert wrongly <= 0.01
    assert after < before
    assert (fill_err <= (R.tol(CLEAN, params) + 2)[filled]).all()


def test_fusion_properties():
    params = SCENARIO[0]
    frames = [R.corrupt(CLEAN, seed) for seed in range(5)]
    d16 = [f[0].astype(np.uint16) for f in frames]
    fused = api.depth_fuse_host(d16, 160, 120, min_frames=3).astype(np.int64)
    never = ~np.any([f[1] | f[2] for f in frames], axis=0)                      # untouched in all five frames
    one_med = api.depth_filter_host(d16[0], 160, 120, **dict(GOOD, fly_min_support=0, radius=1, fill_min=0, min_mm=0, max_mm=0))[0].astype(np.int64)
    alive = never & (fused != 0) & (one_med != 0)
    rms_one, rms_median, rms_fused = rms(frames[0][0], CLEAN, alive), rms(one_med, CLEAN, alive), rms(fused, CLEAN, alive)
    off = lambda d: int(((d != 0) & (np.abs(d - CLEAN) > 20)).sum())            # noqa: E731
    unmeasured = [int((f[0] == 0).sum()) for f in frames]
    out, flags, _ = api.depth_filter_host(fused.astype(np.uint16), 160, 120, want_flags=True, **params)
    print(f"rms one frame {rms_one:.3f} its median {rms_median:.3f} fused {rms_fused:.3f}; unmeasured per frame {unmeasured} fused {int((fused == 0).sum())}; "
          f"off by more than 20: single {[off(f[0]) for f in frames]} fused {off(fused)} fused + filter {off(out.astype(np.int64))}")
    assert rms_fused < rms_median                                               # fusion lowers the rms further than one frame's median does
    assert int((fused == 0).sum()) < min(unmeasured)
    # It does not remove the flying pixels: a pixel at a jump flies in every frame with probability at least 0.5, so in at least three of the five
    # (where the median itself flies) with probability at least 0.5 -- at least half of one frame's number are still there ...
    assert 2 * off(fused) >= min(off(f[0]) for f in frames)
    assert off(out.astype(np.int64)) <= 3                                       # ... the filter on the fused frame does
