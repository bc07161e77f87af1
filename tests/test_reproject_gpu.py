"""Reprojection on the device: pr_depth_reproject_dev against the numpy reference (tests/reproject_ref.py) and the host twin byte for byte -- depth,
source image, counts --, the same call twice, the optional outputs left out, refusals that leave the device buffers untouched, and the hand-over
of a reprojected frame to the stages behind it.  Bytes and hand-over only: tests/test_reproject_host.py holds the definition to what it is for."""
import ctypes as C

import numpy as np
import pytest

import reproject_cases as RC
import reproject_ref as R
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

CASES = RC.cases()
K9 = lambda k: (k[0], 0, k[2], 0, k[1], k[3], 0, 0, 1)                            # noqa: E731


def run_dev(sources, w, h, K, dtype, params, want_source=True):
    res = api.depth_reproject(sources, w, h, K9(K), dtype=dtype, want_source=want_source, **params)
    return tuple(r.to_host().reshape(h, w) if isinstance(r, api.DeviceVector) else r for r in res)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_reference_and_host(gpu, case):
    name, sources, w, h, K, params = case
    dev_sources = RC.api_sources(api, sources, True)
    host_sources = RC.api_sources(api, sources, False)
    for dtype in RC.DTYPES:
        what = f"{name} {np.dtype(dtype).name}"
        ref = R.reproject(RC.ref_sources(sources), w, h, K, dtype, params)
        got = run_dev(dev_sources, w, h, K, dtype, params)
        assert got[0].dtype == dtype and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2], what
        host = api.depth_reproject_host(host_sources, w, h, K9(K), dtype=dtype, want_source=True, **params)
        assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes() and got[2] == host[2], what
        again = run_dev(dev_sources, w, h, K, dtype, params)                    # the same call twice
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2], what
        bare = run_dev(dev_sources, w, h, K, dtype, params, want_source=False)  # source_dev_out NULL
        assert bare[0].tobytes() == got[0].tobytes() and bare[1] == got[2], what


def raw_call(lib, table, n, w, h, K, dtype, params, out, source, counts):
    return lib.pr_depth_reproject_dev(C.addressof(table), n, w, h, K[0], K[1], K[2], K[3], int(dtype == np.int32), C.addressof(params), out, source, counts)


def case_table(name):
    _, sources, w, h, K, params = next(c for c in CASES if c[0] == name)
    dev = RC.api_sources(api, sources, True)
    table = (_lib.ReprojectSourceDesc * len(dev))(*[s.desc(s.data.data()) for s in dev])
    return sources, dev, table, w, h, K, params


def test_null_source_image_and_counts(gpu):
    sources, dev, table, w, h, K, params = case_table("eight_sources")
    for dtype in RC.DTYPES:
        out = api.DeviceVector(w * h, dtype)
        _lib.check(raw_call(_lib.load(), table, len(dev), w, h, K, dtype, api.ReprojectParams(**params), out.data(), None, None))
        assert out.to_host().tobytes() == R.reproject(RC.ref_sources(sources), w, h, K, dtype, params)[0].tobytes()


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_refusals_leave_the_device_buffers(gpu, dtype):
    lib = _lib.load()
    sources, dev, table, w, h, K, params = case_table("67x45_from_61x37_s2_int32")
    before = [d.data.to_host().tobytes() for d in dev]
    out = api.DeviceVector.from_host(np.full(w * h, 0x2BCD, dtype))
    source = api.DeviceVector.from_host(np.full(w * h, 0xEE, np.uint8))
    good = api.ReprojectParams(**params)
    bad = _lib.ReprojectParamsDesc.from_buffer_copy(bytes(good))
    bad.splat = 4
    cnt = _lib.ReprojectCounts()
    C.memset(C.addressof(cnt), 0x5A, 288)
    bad_T = (_lib.ReprojectSourceDesc * 1)(_lib.ReprojectSourceDesc.from_buffer_copy(bytes(table[0])))
    bad_T[0].T[15] = 2.0
    own = (_lib.ReprojectSourceDesc * 1)(_lib.ReprojectSourceDesc.from_buffer_copy(bytes(table[0])))
    assert raw_call(lib, table, 1, w, h, K, dtype, bad, out.data(), source.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert raw_call(lib, table, 1, w, 0, K, dtype, good, out.data(), source.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert raw_call(lib, table, 9, w, h, K, dtype, good, out.data(), source.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert raw_call(lib, bad_T, 1, w, h, K, dtype, good, out.data(), source.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID
    assert raw_call(lib, own, 1, w, h, K, dtype, good, own[0].data, source.data(), C.addressof(cnt)) == _lib.PR_ERR_INVALID      # depth_out is the source
    assert [d.data.to_host().tobytes() for d in dev] == before
    assert (out.to_host() == 0x2BCD).all() and (source.to_host() == 0xEE).all() and bytes(cnt) == b"\x5a" * 288
    # the next call on the same context is not disturbed
    ref = R.reproject(RC.ref_sources(sources), w, h, K, dtype, params)
    got = run_dev(dev, w, h, K, dtype, params)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]


# ---- the hand-over at the workload's size -----------------------------------------------------------------------------------------------------
def test_hand_over_cloud_to_scorers(gpu, scenario, model):
    """The golden obj_06 frame as a bare cloud and back into a frame: the scorers cannot tell the difference."""
    W, H, K = synth.WIDTH, synth.HEIGHT, scenario["K"]
    frame = np.ascontiguousarray(scenario["depth"][1], np.int32)
    src = api.DeviceVector.from_host(frame.reshape(-1))
    cloud = api.depth2cloud(src, W, H, K)
    assert cloud.size() == 3 * int((frame > 0).sum())
    back, counts = api.cloud_to_depth(cloud, W, H, K, dtype=np.int32)
    assert back.to_host().tobytes() == frame.tobytes() and counts["kept"] == counts["sources"][0]["samples"] == cloud.size() // 3
    poses = synth.hypotheses(8)
    want = api.score_poses(model, poses, W, H, scenario["proj"], src, 5)
    assert api.score_poses(model, poses, W, H, scenario["proj"], back, 5).tobytes() == want.tobytes()
    back16, _ = api.cloud_to_depth(cloud, W, H, K)                               # uint16, the default
    assert back16.dtype == np.uint16 and api.score_poses(model, poses, W, H, scenario["proj"], back16, 5).tobytes() == want.tobytes()
    segs, labels, seg_counts = api.scene_segments(back, W, H, jump_mm=20)
    assert labels.size() == W * H and seg_counts[0] >= 1
    scene = api.Scene_projective().init_Scene_projective_device(back, K, W, H)
    assert scene.pcd_buffer.size() == 3 * W * H


def test_hand_over_mixed_sources_to_depth_filter(gpu):
    """Two frames of different sizes and a cloud into a 640 x 480 int32 target, then the fill."""
    W, H = 640, 480
    K = (600.0, 600.0, 319.5, 239.5)
    a = RC.src_frame(320, 240, seed=1)
    b = np.clip(RC.src_frame(641, 479, seed=2), 0, 65535)
    sources = [R.frame(a.astype(np.int32), (300.0, 300.0, 159.5, 119.5), RC.rigid(ry=4.0, t=(0.05, 0, 0))),
               R.frame(b.astype(np.uint16), (601.0, 599.0, 320.0, 239.0), RC.rigid(rx=-3.0, t=(0, 0.02, 0.01))), R.cloud(RC.src_cloud(50000, seed=3), RC.rigid(rz=2.0))]
    params = dict(splat=2, min_mm=200, tol_mm=10, tol_permille=5, occl_radius=2, occl_min_front=4)
    made = [api.ReprojectSource.frame(sources[0]["data"], 320, 240, K9(sources[0]["K"]), sources[0]["T"]),
            api.ReprojectSource.frame(sources[1]["data"], 641, 479, K9(sources[1]["K"]), sources[1]["T"]), api.ReprojectSource.cloud(sources[2]["data"], sources[2]["T"])]
    out, source, counts = api.depth_reproject(made, W, H, K9(K), dtype=np.int32, want_source=True, **params)
    ref = R.reproject(sources, W, H, K, np.int32, params)
    assert out.to_host().tobytes() == ref[0].tobytes() and source.to_host().tobytes() == ref[1].tobytes() and counts == ref[2]
    assert all(s["won"] > 0 for s in counts["sources"]) and counts["hidden"] > 0
    fill = dict(tol_mm=10, tol_permille=5, radius=1, fill_min=5)
    filled, fcounts = api.depth_filter(out, W, H, **fill)
    host = api.depth_filter_host(ref[0], W, H, **fill)
    assert filled.to_host().tobytes() == host[0].tobytes() and fcounts == host[1] and fcounts[api.DEPTH_FILLED] > 0
