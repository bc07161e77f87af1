"""Host-side mirror of the reference's public API for the hot path, on top of the C ABI.

Names, argument meaning and error behaviour follow the reference headers so that tests read like
the reference's own drivers (``test.cpp``, ``cuda_renderer/test.cpp``):

  cuda_renderer::Model / compute_proj / render / render_host        cuda_renderer/renderer.h:27-248
  cuda_icp::depth2cloud / ICP_Point2Plane / RegistrationResult /
            ICPConvergenceCriteria                                  cuda_icp/icp.h:26-120
  ::Scene_projective / ::Scene_nn / KDTree_cuda                     cuda_icp/scene/**.h
  ::device_vector_holder<T>                                         cuda_icp/scene/common.h:16-44

The C++ adapters in include/cuda_renderer and include/cuda_icp are the compiled drop-in; this module
is the same surface for python callers (tests, bench.py).  Everything that touches the device goes
through libpose_refine_hip.so -- nothing here computes on the CPU except what the reference also
computes on the CPU (model import, scene preparation).
"""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (CloudCounts, CloudParamsDesc, COMM_ID_BYTES, DEPTH_FILLED, DEPTH_FILTER_MAX_RADIUS, DEPTH_FLYING, DEPTH_FUSE_MAX, DEPTH_GATED, DEPTH_KEPT, DEPTH_SMOOTHED, DEPTH_UNMEASURED, DepthFilterCounts, DepthFilterParamsDesc, COMPOSE_MAX_POSES, COMPOSE_NONE, CONTOUR, CONTOUR_FIT, CONTOUR_MAX_RADIUS, EDGE_NONE, COVER, COVER_ACCEPTED, COVER_EMPTY, COVER_FRAME, COVER_NOT_IN_ORDER, COVER_NO_POSITION, COVER_REASON_CAP, COVER_REASON_THRESHOLD, COVER_REJECTED, COVER_STATE_MASK, Criteria, FRAME, KDNODE, KNN_MAX_K, KNN_NONE, MeshRef, NORMAL, NORMAL_MAX_STEP, PAIR_SOLID, PENETRATION_MAX_POSES, PLANE, PLANE_BEHIND, PLANE_MAX_CANDIDATES, PLANE_MAX_PLANES, PLANE_MAX_SAMPLES, PLANE_NO_DEPTH, PlaneParamsDesc, POSE_DIST, POSE_DIST_MAX_POSES, POSE_DIST_MAX_SYMS, PPF_ENTRY, PPF_MAX_CELLS, PPF_MAX_MODEL_POINTS, PPF_MAX_MODELS, PPF_MAX_PEAKS, PPF_MAX_SCENE_POINTS, PPF_PEAK, PPFModelDesc, PPFParams, PyramidLevel as _PyramidLevel, RESULT, ROBUST_CAUCHY, ROBUST_HUBER, ROBUST_NONE, ROBUST_TUKEY, RobustDesc, Roi, SCENE_GRID, SCENE_NN, SCENE_PROJ, SCENE_PROJ_CROP, SCORE, SEGMENT, SEGMENT_DROPPED, SEGMENT_MAX, SEGMENT_MAX_ROOTS, SegmentParamsDesc, SOLVE_DEVICE, SOLVE_HOST, VISIBLE, VSD, VSD_MAX_TAUS,
                   PoseRefineError, SceneGridDesc, SceneNNDesc, SceneProjCropDesc, SceneProjDesc, check, ptr)
from ._lib import (REPROJECT_HIDDEN, REPROJECT_MAX_RADIUS, REPROJECT_MAX_SOURCES, REPROJECT_NONE, SRC_CLOUD, SRC_DEPTH_I32, SRC_DEPTH_U16,  # noqa: F401
                   ReprojectCounts, ReprojectParamsDesc, ReprojectSourceDesc)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


# ------------------------------------------------------------------------------------------------
# library / options
# ------------------------------------------------------------------------------------------------
def init(device: int = 0):
    check(_lib.load().pr_init(device))


def set_device(device: int):
    """Bind the calling thread to the shared context of ``device`` (one host thread per GPU)."""
    check(_lib.load().pr_set_device(device))


def shutdown():
    """``pr_shutdown``: release the calling thread's context (workspaces, streams, communicator).  Device buffers handed out by
    this module (DeviceVector, Model, scenes) stay valid; the next call re-creates the context."""
    _slots().clear()
    check(_lib.load().pr_shutdown())


def thread_context(enable: bool = True):
    """Private context (own stream / workspaces) for the calling thread: the reference's "many host threads,
    each driving its own pose" usage (README.md:15) without queueing on the device's shared context."""
    check(_lib.load().pr_thread_context(1 if enable else 0))


def invalidate(dev_ptr: int, nbytes: int = 0):
    """Announce a write to device memory the library could not see (drops derived scene data cached by address)."""
    check(_lib.load().pr_invalidate(int(dev_ptr), int(nbytes)))


def device_count() -> int:
    return _lib.load().pr_device_count()


# ---- the job's one collective (C ABI over RCCL) -------------------------------------------------------------------------
def comm_id() -> bytes:
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    check(_lib.load().pr_comm_id(buf))
    return bytes(buf)


def comm_init_rank(comm_id_bytes: bytes, rank: int, world: int):
    buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(comm_id_bytes)
    check(_lib.load().pr_comm_init_rank(buf, rank, world))


def comm_init_all(n_devices: int):
    check(_lib.load().pr_comm_init_all(n_devices))


def comm_destroy():
    check(_lib.load().pr_comm_destroy())


def comm_rank():
    r, w = C.c_int(), C.c_int()
    check(_lib.load().pr_comm_rank(C.byref(r), C.byref(w)))
    return r.value, w.value


def gather_results(send_dev: int, n_local: int, n_total: int, root: int = 0, recv_dev: Optional[int] = None):
    """``pr_gather_results``: this rank's shard (device memory) -> ``recv_dev`` on root, global hypothesis order.
    Enqueued on the context's stream."""
    check(_lib.load().pr_gather_results(int(send_dev) if send_dev else None, n_local, n_total, root, int(recv_dev) if recv_dev else None))


def sync():
    check(_lib.load().pr_sync())


def set_option(name: str, value: int):
    check(_lib.load().pr_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_int()
    check(_lib.load().pr_get_option(name.encode(), C.byref(v)))
    return v.value


def profile_reset():
    check(_lib.load().pr_profile_reset())


def profile_read():
    ms, rms, cms = C.c_double(), C.c_double(), C.c_double()
    n, pts, nbytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(_lib.load().pr_profile_read(C.byref(ms), C.byref(n), C.byref(pts), C.byref(nbytes), C.byref(rms), C.byref(cms)))
    return dict(icp_kernel_ms=ms.value, icp_launches=n.value, icp_points=pts.value, icp_bytes=nbytes.value,
                render_ms=rms.value, cloud_ms=cms.value)


def profile_launches() -> np.ndarray:
    """``pr_profile_launches``: the timed correspondence launches since the last reset, one by one, in microseconds."""
    n = C.c_uint32()
    check(_lib.load().pr_profile_launches(None, 0, C.byref(n)))
    out = np.zeros(n.value, np.float32)
    if n.value:
        check(_lib.load().pr_profile_launches(ptr(out), n.value, C.byref(n)))
    return out


def profile_nn():
    """``pr_profile_nn``: accumulated time of the four kernels of the timed kd-tree passes -- (ms[4]: search, bound, task walk, winners pass; passes)."""
    ms = np.zeros(4, np.float64)
    n = C.c_uint64()
    check(_lib.load().pr_profile_nn(ptr(ms), C.byref(n)))
    return ms, n.value


def stats():
    """``pr_stats``: (asynchronous batches repeated by the stale-cache safety net, timings dropped after a failed event call)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(_lib.load().pr_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


def mesh_order(tris) -> np.ndarray:
    """``pr_debug_mesh_order``: the permutation (uint32, place -> triangle index) of the library's ordered copy of a (T, 3, 3) float32 soup.  No device needed."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    perm = np.empty(len(t), np.uint32)
    check(_lib.load().pr_debug_mesh_order(t.ctypes.data, len(t), perm.ctypes.data))
    return perm


def mesh_fingerprint(tris) -> int:
    """``pr_debug_mesh_fingerprint``: the order-independent 64-bit fingerprint of a (T, 3, 3) float32 soup.  No device needed."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    v = C.c_uint64()
    check(_lib.load().pr_debug_mesh_fingerprint(t.ctypes.data, len(t), C.byref(v)))
    return v.value


def tight_box(tris, pose, width: int, height: int, proj, roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_debug_tight_box``: (tight, loose) pixel boxes ``[x0, y0, x1, y1]`` (int32, raster coordinates, inclusive) of a (T, 3, 3) float32
    soup under one pose -- what the asynchronous path's box kernel leaves for the hypothesis, and the host's box it started from.  No device needed."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    m = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
    pj = np.ascontiguousarray(proj, dtype=np.float32).reshape(16)
    tight, loose = np.empty(4, np.int32), np.empty(4, np.int32)
    check(_lib.load().pr_debug_tight_box(t.ctypes.data, len(t), m.ctypes.data, pj.ctypes.data, width, height, Roi(*roi),
                                         tight.ctypes.data, loose.ctypes.data))
    return tight, loose


def box_layout(box, width: int, height: int, bands: bool, xs=(), rows=()):
    """``pr_debug_box_layout``: (slot ints, offsets) of the depth box ``[x0, y0, x1, y1]`` (raster coordinates, inclusive) of a width x height
    frame in the asynchronous path's workspace, banded (four image rows interleaved) or row-major; offsets (uint32) of the pixels
    (xs[i], image row rows[i]) from the start of the slot.  No device needed."""
    b = np.ascontiguousarray(box, dtype=np.int32).reshape(4)
    x = np.ascontiguousarray(xs, dtype=np.int32).reshape(-1)
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    if len(x) != len(r):
        raise ValueError("xs and rows differ in length")
    slot, off = C.c_uint32(), np.empty(len(x), np.uint32)
    check(_lib.load().pr_debug_box_layout(b.ctypes.data, width, height, 1 if bands else 0, x.ctypes.data, r.ctypes.data, len(x),
                                          C.byref(slot), off.ctypes.data))
    return slot.value, off


def gather_profile():
    """HIP-event time of the gathers issued while option ``profile`` was on: (total ms, count).  Waits for the library stream."""
    ms, n = C.c_double(), C.c_uint64()
    check(_lib.load().pr_gather_profile(C.byref(ms), C.byref(n)))
    return ms.value, n.value


def nn_counters(passes: int = 21) -> np.ndarray:
    """Per-pass work counters of the kd-tree search kernels (option ``nn_count``): (passes, 8) uint64, the columns of
    ``enum NNCounter`` (csrc/nn_search.hip) -- 0 kCntQueries, 1 kCntWindow (settled by the pixel window), 2 kCntTree (handed to a tree
    walk), 3 kCntDescents (pyramid descents), 4 kCntNodes, 5 kCntLeaves, 6 kCntLeafPoints, 7 kCntCells (window cells read)."""
    out = np.zeros((passes, 8), np.uint64)
    check(_lib.load().pr_nn_counters(ptr(out), passes))
    return out


def shard_range(n_items: int, rank: int, world: int):
    first, count = C.c_uint32(), C.c_uint32()
    _lib.load().pr_shard_range(n_items, rank, world, C.byref(first), C.byref(count))
    return first.value, count.value


# ------------------------------------------------------------------------------------------------
# device_vector_holder<T>
# ------------------------------------------------------------------------------------------------
class DeviceVector:
    """RAII device buffer (``device_vector_holder<T>``: common.h:16-44 / renderer.h:161-187)."""

    def __init__(self, count: int = 0, dtype=np.float32, _adopt: Optional[int] = None):
        self.dtype = np.dtype(dtype)
        self.count = int(count)
        self._ptr = None
        if _adopt is not None:
            self._ptr = int(_adopt)
        elif count > 0:
            p = C.c_void_p()
            check(_lib.load().pr_malloc(C.byref(p), self.count * self.dtype.itemsize))
            self._ptr = p.value

    @classmethod
    def from_host(cls, arr: np.ndarray, dtype=None) -> "DeviceVector":
        arr = np.ascontiguousarray(arr, dtype=dtype)
        dv = cls(arr.size if arr.dtype.fields is None else arr.shape[0], arr.dtype)
        if arr.nbytes:
            check(_lib.load().pr_memcpy_h2d(dv._ptr, ptr(arr), arr.nbytes))
        return dv

    def data(self) -> int:
        return self._ptr or 0

    def size(self) -> int:
        return self.count

    def to_host(self) -> np.ndarray:
        out = np.empty(self.count, self.dtype)
        if self.count:
            check(_lib.load().pr_memcpy_d2h(ptr(out), self._ptr, out.nbytes))
        return out

    def free(self):
        if self._ptr:
            _lib.load().pr_free(self._ptr)
            self._ptr = None
            self.count = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# cuda_renderer
# ------------------------------------------------------------------------------------------------
class Model:
    """``cuda_renderer::Model(fileName)`` (renderer.cpp:11-104): ``tris`` feeds the path; ``vertices``, ``faces``,
    ``bbox_min`` / ``bbox_max`` are the reference's other public members (renderer.h:143-147)."""

    def __init__(self, file_name: Optional[str] = None, tris: Optional[np.ndarray] = None):
        if tris is not None:
            self.tris = _f32(tris, (-1, 3, 3))
            self.vertices = self.tris.reshape(-1, 3)
            self.faces = np.arange(len(self.vertices), dtype=np.int32).reshape(-1, 3)
            self.bbox_min, self.bbox_max = (self.vertices.min(0), self.vertices.max(0)) if len(self.vertices) else (np.zeros(3, np.float32),) * 2
        else:
            lib = _lib.load()
            nt, nv = C.c_size_t(), C.c_size_t()
            check(lib.pr_mesh_count(file_name.encode(), C.byref(nt), C.byref(nv)))
            buf = np.zeros((nt.value, 3, 3), np.float32)
            self.vertices = np.zeros((nv.value, 3), np.float32)
            self.faces = np.zeros((nt.value, 3), np.int32)
            self.bbox_min, self.bbox_max = np.zeros(3, np.float32), np.zeros(3, np.float32)
            check(lib.pr_mesh_load(file_name.encode(), ptr(buf), nt.value, C.byref(nt), ptr(self.vertices), nv.value, C.byref(nv),
                                   ptr(self.faces), ptr(self.bbox_min), ptr(self.bbox_max)))
            self.tris = buf
        self._dev: Optional[DeviceVector] = None
        self._dev_vertices: Optional[DeviceVector] = None

    def device_tris(self) -> DeviceVector:
        """Triangles resident on the device (the ``device_vector_holder<Triangle>`` overloads)."""
        if self._dev is None:
            self._dev = DeviceVector.from_host(self.tris.reshape(-1), np.float32)
        return self._dev

    def device_vertices(self) -> DeviceVector:
        """``vertices`` resident on the device (3 float32 each): the points ``pose_distance`` measures with.  A file's vertex list as it
        is (each vertex once); for a model made from ``tris=`` the triangle corners as they are."""
        if self._dev_vertices is None:
            self._dev_vertices = DeviceVector.from_host(_f32(self.vertices, -1), np.float32)
        return self._dev_vertices


def compute_proj(K, width: int, height: int, near: float = 10.0, far: float = 10000.0) -> np.ndarray:
    out = np.zeros(16, np.float32)
    k = _f32(K, -1)
    _lib.load().pr_compute_proj(ptr(k), width, height, near, far, ptr(out))
    return out


def _tris_dev(tris) -> DeviceVector:
    if isinstance(tris, Model):
        return tris.device_tris()
    if isinstance(tris, DeviceVector):
        return tris
    return DeviceVector.from_host(_f32(tris, -1))


def render(tris, poses, width: int, height: int, proj, roi: Sequence[int] = (0, 0, 0, 0)) -> DeviceVector:
    """``cuda_renderer::render`` -> ``render_cuda_keep_in_gpu`` (renderer.cu:269-336): int32 depth in mm
    for every pose, kept on the device, 0 where nothing was drawn."""
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    rw, rh = (roi[2], roi[3]) if roi[2] > 0 and roi[3] > 0 else (width, height)
    out = DeviceVector(len(poses) * rw * rh, np.int32)
    pj = _f32(proj, -1)
    check(_lib.load().pr_render(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), Roi(*roi), out.data()))
    return out


def render_span(tris, poses, width: int, height: int, proj, roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_render_span``: ``render`` with the far surface.  Returns (near, far) device vectors of int32 mm: ``near`` is ``render``'s bytes,
    ``far`` the largest fragment depth of every pixel, 0 where nothing was drawn."""
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    rw, rh = (roi[2], roi[3]) if roi[2] > 0 and roi[3] > 0 else (width, height)
    near, far = DeviceVector(len(poses) * rw * rh, np.int32), DeviceVector(len(poses) * rw * rh, np.int32)
    pj = _f32(proj, -1)
    check(_lib.load().pr_render_span(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), Roi(*roi), near.data(), far.data()))
    return near, far


def raw2depth_mask(raw: DeviceVector, want_depth: bool = True, want_mask: bool = True):
    """``raw2depth_uint16_cuda`` / ``raw2mask_uint8_cuda`` / ``raw2depth_mask_cuda`` (renderer.cu:338-439) for a whole
    render stack: returns (uint16 depth or None, uint8 mask or None) as flat host arrays."""
    n = raw.size()
    d = np.empty(n, np.uint16) if want_depth else None
    m = np.empty(n, np.uint8) if want_mask else None
    check(_lib.load().pr_raw2depth_mask(raw.data(), n, ptr(d) if want_depth else None, ptr(m) if want_mask else None))
    return d, m


def render_host(tris, poses, width: int, height: int, proj, roi: Sequence[int] = (0, 0, 0, 0)) -> np.ndarray:
    """``cuda_renderer::render_host`` -> ``render_cuda`` (renderer.cu:189-267): result on the host."""
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    rw, rh = (roi[2], roi[3]) if roi[2] > 0 and roi[3] > 0 else (width, height)
    out = np.empty((len(poses), rh, rw), np.int32)
    pj = _f32(proj, -1)
    check(_lib.load().pr_render_to_host(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), Roi(*roi), ptr(out)))
    return out


# ------------------------------------------------------------------------------------------------
# cuda_icp
# ------------------------------------------------------------------------------------------------
@dataclass
class ICPConvergenceCriteria:           # icp.h:38-50
    relative_fitness: float = 1e-5
    relative_rmse: float = 1e-5
    max_iteration: int = 30

    def c(self) -> Criteria:
        return Criteria(self.relative_fitness, self.relative_rmse, self.max_iteration)


@dataclass
class RegistrationResult:               # icp.h:26-36
    transformation_: np.ndarray
    inlier_rmse_: float
    fitness_: float

    @classmethod
    def from_record(cls, r) -> "RegistrationResult":
        return cls(np.array(r["T"], np.float32).reshape(4, 4), float(r["inlier_rmse"]), float(r["fitness"]))


def depth2cloud(depth_dev, width: int, height: int, K, stride: int = 1, tl_x: int = 0, tl_y: int = 0,
                dtype=np.int32, offset_elems: int = 0) -> DeviceVector:
    """``cuda_icp::depth2cloud_cuda<T>`` (icp.cu:256-291): DEVICE depth pointer in, device cloud out.
    ``depth_dev`` is a DeviceVector (or raw device address); offset_elems selects an image of a stack."""
    base = depth_dev.data() if isinstance(depth_dev, DeviceVector) else int(depth_dev)
    dt = np.dtype(dtype)
    if isinstance(depth_dev, DeviceVector) and (offset_elems + width * height) * dt.itemsize > depth_dev.size() * depth_dev.dtype.itemsize:
        raise ValueError(f"depth buffer of {depth_dev.size()} {depth_dev.dtype} values holds no {width} x {height} {dt} image at element {offset_elems}")
    k = _f32(K, -1)
    out, n = C.c_void_p(), C.c_uint32()
    fn = _lib.load().pr_depth2cloud_u16 if dt == np.uint16 else _lib.load().pr_depth2cloud_i32
    check(fn(base + offset_elems * dt.itemsize, width, height, ptr(k), stride, tl_x, tl_y, C.byref(out), C.byref(n)))
    return DeviceVector(n.value * 3, np.float32, _adopt=out.value)


class Scene_projective:
    """``::Scene_projective`` (depth_scene.h:7-48) initialised like ``init_Scene_projective_cuda``
    (depth_scene.cu:3-20): CPU preparation (back-projection + normals), then two uploads."""

    def __init__(self):
        self.width, self.height, self.max_dist_diff = 640, 480, 0.1
        self.K = np.zeros(9, np.float32)
        self.pcd_buffer: Optional[DeviceVector] = None
        self.normal_buffer: Optional[DeviceVector] = None
        self.pcd_host = self.normal_host = None

    def init_Scene_projective_cuda(self, scene_depth: np.ndarray, scene_K, width: int = 640, height: int = 480,
                                   max_dist_diff: float = 0.1):
        if scene_depth.dtype not in (np.uint16, np.int32):          # depth_scene.cpp:11-12 assert
            raise ValueError("scene depth must be CV_16U or CV_32S")
        # the reference reads scene_depth.at(r, c) for r < height, c < width (depth_scene.cpp:17-30) and trusts the caller; an image
        # of another size than the (width, height) given -- the defaults are 640 x 480 as in depth_scene.h -- is an error here
        if scene_depth.ndim != 2 or scene_depth.shape != (height, width):
            raise ValueError(f"scene depth is {scene_depth.shape}, expected ({height}, {width}): pass width / height of the image")
        self.width, self.height, self.max_dist_diff = width, height, max_dist_diff
        self.K = _f32(scene_K, -1)
        d = np.ascontiguousarray(scene_depth)
        pcd = np.zeros((width * height, 3), np.float32)
        nrm = np.zeros((width * height, 3), np.float32)
        check(_lib.load().pr_scene_proj_prepare(ptr(d), int(d.dtype == np.int32), ptr(self.K), width, height, ptr(pcd), ptr(nrm)))
        self.pcd_host, self.normal_host = pcd, nrm
        self.pcd_buffer = DeviceVector.from_host(pcd.reshape(-1))
        self.normal_buffer = DeviceVector.from_host(nrm.reshape(-1))
        return self

    def init_Scene_projective_device(self, scene_depth_dev: "DeviceVector", scene_K, width: int = 640, height: int = 480,
                                     max_dist_diff: float = 0.1):
        """the same initialisation with the depth image already on the device and the
        preparation (back-projection + normals) done by a kernel -- no CPU work, no PCIe traffic."""
        if scene_depth_dev.dtype not in (np.uint16, np.int32):
            raise ValueError("scene depth must be CV_16U or CV_32S")
        if scene_depth_dev.size() != width * height:
            raise ValueError(f"scene depth holds {scene_depth_dev.size()} values, expected {width} x {height}: pass width / height of the image")
        self.width, self.height, self.max_dist_diff = width, height, max_dist_diff
        self.K = _f32(scene_K, -1)
        if self.pcd_buffer is None or self.pcd_buffer.size() != width * height * 3:        # a scene object that is re-initialised frame after frame keeps its arrays
            self.pcd_buffer = DeviceVector(width * height * 3, np.float32)
            self.normal_buffer = DeviceVector(width * height * 3, np.float32)
        check(_lib.load().pr_scene_proj_prepare_dev(scene_depth_dev.data(), int(scene_depth_dev.dtype == np.int32), ptr(self.K),
                                                    width, height, self.pcd_buffer.data(), self.normal_buffer.data()))
        return self

    kind = SCENE_PROJ
    tl_x = tl_y = 0

    def desc(self):
        view = SceneProjDesc(self.width, self.height, self.max_dist_diff, (C.c_float * 9)(*self.K),
                             self.pcd_buffer.data(), self.normal_buffer.data())
        if self.kind == SCENE_PROJ_CROP:
            return SceneProjCropDesc(view, self.tl_x, self.tl_y)
        return view

    def crop(self, window: Sequence[int]) -> "Scene_projective":
        """The same scene restricted to ``window`` = (x, y, width, height): arrays of the window's size and the
        ``tl_x / tl_y`` offsets of pcd2dep / dep2pcd (common.h:47-73) -- SURVEY 8f rank 3."""
        x, y, w, h = (int(v) for v in window)
        out = Scene_projective()
        out.kind = SCENE_PROJ_CROP
        out.width, out.height, out.max_dist_diff, out.K = w, h, self.max_dist_diff, self.K
        out.tl_x, out.tl_y = x, y
        out.pcd_buffer = DeviceVector(w * h * 3, np.float32)
        out.normal_buffer = DeviceVector(w * h * 3, np.float32)
        check(_lib.load().pr_scene_proj_crop_dev(self.pcd_buffer.data(), self.normal_buffer.data(), self.width, self.height,
                                                 Roi(x, y, w, h), out.pcd_buffer.data(), out.normal_buffer.data()))
        return out


class Scene_nn:
    """``::Scene_nn`` + ``KDTree_cuda`` (pcd_scene.h:27-137) initialised like ``init_Scene_nn_cuda``
    (pcd_scene.cu:3-20): CPU normals + kd-tree build, then three uploads."""

    kind = SCENE_NN

    def __init__(self):
        self.max_dist_diff = 0.1
        self.pcd_buffer = self.normal_buffer = self.nodes = None
        self.pcd_host = self.normal_host = self.nodes_host = None
        self.camera = None                                          # (fx, fy, cx, cy, w, h) of the depth image the scene was made from, if known

    def init_Scene_nn_cuda(self, scene_depth: np.ndarray, scene_K, max_leaf: int = 10, max_dist_diff: float = 0.1):
        if scene_depth.dtype not in (np.uint16, np.int32):          # pcd_scene.cpp:6-7 assert
            raise ValueError("scene depth must be CV_16U or CV_32S")
        h, w = scene_depth.shape
        k = _f32(scene_K, -1)
        d = np.ascontiguousarray(scene_depth)
        pcd = np.zeros((w * h, 3), np.float32)
        nrm = np.zeros((w * h, 3), np.float32)
        nodes = np.zeros(2 * w * h + 1, KDNODE)
        npts, nnodes = C.c_uint32(), C.c_uint32()
        check(_lib.load().pr_scene_nn_prepare(ptr(d), int(d.dtype == np.int32), ptr(k), w, h, max_leaf, ptr(pcd), ptr(nrm),
                                              ptr(nodes), len(nodes), C.byref(npts), C.byref(nnodes)))
        self.max_dist_diff = max_dist_diff
        self.camera = (float(k[0]), float(k[4]), float(k[2]), float(k[5]), int(w), int(h))
        self.pcd_host = np.ascontiguousarray(pcd[:npts.value])
        self.normal_host = np.ascontiguousarray(nrm[:npts.value])
        self.nodes_host = np.ascontiguousarray(nodes[:nnodes.value])
        self.pcd_buffer = DeviceVector.from_host(self.pcd_host.reshape(-1))
        self.normal_buffer = DeviceVector.from_host(self.normal_host.reshape(-1))
        self.nodes = DeviceVector.from_host(self.nodes_host)
        return self

    def init_Scene_nn_device(self, scene_depth_dev: "DeviceVector", scene_K, width: int, height: int, max_leaf: int = 10,
                             max_dist_diff: float = 0.1):
        """normals, valid-pixel gather and the level-order kd-tree build all on the device."""
        k = _f32(scene_K, -1)
        px = width * height
        if scene_depth_dev.size() != px:
            raise ValueError(f"scene depth holds {scene_depth_dev.size()} values, expected {width} x {height}")
        if self.pcd_buffer is None or self.pcd_buffer.size() != px * 3 or self.nodes is None or self.nodes.size() != 2 * px + 1:    # (kept across re-initialisations)
            self.pcd_buffer = DeviceVector(px * 3, np.float32)
            self.normal_buffer = DeviceVector(px * 3, np.float32)
            self.nodes = DeviceVector(2 * px + 1, KDNODE)
        npts, nnodes = C.c_uint32(), C.c_uint32()
        check(_lib.load().pr_scene_nn_prepare_dev(scene_depth_dev.data(), int(scene_depth_dev.dtype == np.int32), ptr(k), width, height, max_leaf,
                                                  self.pcd_buffer.data(), self.normal_buffer.data(), self.nodes.data(), 2 * px + 1,
                                                  C.byref(npts), C.byref(nnodes)))
        self.max_dist_diff = max_dist_diff
        self.camera = (float(k[0]), float(k[4]), float(k[2]), float(k[5]), int(width), int(height))
        self._n_points, self._n_nodes = npts.value, nnodes.value
        self.pcd_host = self.normal_host = self.nodes_host = None
        return self

    def init_Scene_nn_cloud(self, points, k: int = 16, max_radius: float = float("inf"), viewpoint=(0.0, 0.0, 0.0), max_leaf: int = 10,
                            max_dist_diff: float = 0.1, min_neighbours: int = 3, line_ratio: float = 1e-4):
        """A scene from an unorganised point cloud (``pr_scene_nn_from_cloud_dev``; no counterpart in the reference): ``points`` is an (n, 3)
        float32 host array or a ``DeviceVector`` of 3 n floats, in metres, finite.  The kd-tree is built on the device (the points are reordered:
        a ``DeviceVector`` handed in is adopted and reordered in place), then every point gets the PCA normal of its ``k`` nearest neighbours
        within ``max_radius``, facing ``viewpoint``; a point with fewer than ``min_neighbours`` neighbours, or whose neighbours lie on a line
        (``line_ratio``), keeps (0, 0, 0) and takes no part in ICP or voting.  ``self.cloud_counts`` holds the four counts.  No camera: the
        scene carries no pixel-grid hint."""
        params = CloudParams(k, max_radius, min_neighbours, line_ratio, viewpoint)
        if isinstance(points, DeviceVector):
            if points.size() == 0 or points.size() % 3 or points.dtype != np.float32:
                raise ValueError("points: a DeviceVector of 3 n float32 values, n >= 1")
            self.pcd_buffer = points
        else:
            host = _f32(points)
            if host.ndim != 2 or host.shape[1] != 3 or len(host) == 0:
                raise ValueError("points: an (n, 3) float32 array, n >= 1")
            self.pcd_buffer = DeviceVector.from_host(host.reshape(-1))
        n = self.pcd_buffer.size() // 3
        self.normal_buffer = DeviceVector(n * 3, np.float32)
        self.nodes = DeviceVector(2 * n + 1, KDNODE)
        nnodes, counts = C.c_uint32(), CloudCounts()
        check(_lib.load().pr_scene_nn_from_cloud_dev(self.pcd_buffer.data(), n, max_leaf, C.addressof(params), self.normal_buffer.data(), self.nodes.data(),
                                                     2 * n + 1, C.byref(nnodes), C.addressof(counts)))
        self.max_dist_diff = max_dist_diff
        self.camera = None
        self._n_points, self._n_nodes = n, nnodes.value
        self.pcd_host = self.normal_host = self.nodes_host = None
        self.cloud_counts = _cloud_counts(counts)
        return self

    def desc(self) -> SceneNNDesc:
        n_pts = len(self.pcd_host) if self.pcd_host is not None else self._n_points
        n_nodes = len(self.nodes_host) if self.nodes_host is not None else self._n_nodes
        cam = self.camera if getattr(self, "camera", None) else (0.0, 0.0, 0.0, 0.0, 0, 0)
        return SceneNNDesc(self.max_dist_diff, self.pcd_buffer.data(), self.normal_buffer.data(), self.nodes.data(), n_pts, n_nodes, *cam,
                           _lib.SCENE_NN_CAM_MAGIC if cam[4] else 0)


class Scene_grid:
    """Closest-point grid of a ``Scene_nn`` (``pr_scene_grid``; no counterpart in the reference): every cell of a voxel field over the scene's
    volume holds the scene point nearest to its centre, found once by the exact kd-tree search; an ICP query is then one lookup.  The returned
    point is at most ``sqrt(3) * cell`` farther away than the true nearest one.  Owns its two device buffers; accepted wherever ``Scene_nn`` is."""

    kind = SCENE_GRID

    def __init__(self):
        self._desc = SceneGridDesc()
        self.cell_buffer = self.rec_buffer = None
        self.max_dist_diff = 0.0

    @classmethod
    def from_scene_nn(cls, scene_nn: "Scene_nn", cell: float, reach: Optional[float] = None, lo=None, hi=None, margin: Optional[float] = None) -> "Scene_grid":
        """Box: ``lo`` / ``hi`` (each defaults to the scene points' bounding box grown by ``margin``, default ``max_dist_diff``), shrunk about its
        centre, with a warning, if it would hold more than ``GRID_MAX_CELLS`` cells.  ``reach`` defaults to ``max_dist_diff + (sqrt(3) / 2) * cell``:
        no query with a true neighbour inside ``max_dist_diff - (sqrt(3) / 2) * cell`` then lands in an empty cell."""
        nn = scene_nn.desc()
        mdd = float(scene_nn.max_dist_diff)
        cell = float(cell)
        if not (cell > 0.0 and np.isfinite(cell)):
            raise ValueError("cell must be finite and positive")
        if lo is None or hi is None:
            pts = scene_nn.pcd_host if scene_nn.pcd_host is not None else scene_nn.pcd_buffer.to_host()[:nn.n_points * 3].reshape(-1, 3)
            if len(pts) == 0:
                raise ValueError("the scene has no points")
            m = mdd if margin is None else float(margin)
            lo = pts.min(axis=0).astype(np.float64) - m if lo is None else lo
            hi = pts.max(axis=0).astype(np.float64) + m if hi is None else hi
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        cells = lambda a, b: float(np.prod(np.floor((b - a) / cell) + 1.0))
        if np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi >= lo) and cells(lo, hi) > _lib.GRID_MAX_CELLS:
            import warnings
            want = cells(lo, hi)
            while cells(lo, hi) > _lib.GRID_MAX_CELLS:
                c, half = (lo + hi) / 2, (hi - lo) / 2 * 0.98
                lo, hi = c - half, c + half
            warnings.warn(f"Scene_grid: a box of {want:.3g} cells of {cell} m exceeds GRID_MAX_CELLS = {_lib.GRID_MAX_CELLS}; shrunk about its centre to "
                          f"{lo.tolist()} .. {hi.tolist()}", RuntimeWarning, stacklevel=2)
        out = cls()
        out.max_dist_diff = mdd
        r = mdd + 0.5 * np.sqrt(3.0) * cell if reach is None else float(reach)
        lo32, hi32 = _f32(lo, -1), _f32(hi, -1)
        check(_lib.load().pr_scene_grid_describe(ptr(lo32), ptr(hi32), cell, mdd, r, C.addressof(out._desc)))
        d = out._desc
        out.cell_buffer = DeviceVector(int(d.dim[0]) * int(d.dim[1]) * int(d.dim[2]), np.uint32)
        out.rec_buffer = DeviceVector(int(nn.n_points) * 8, np.float32)
        check(_lib.load().pr_scene_grid_build_dev(C.addressof(nn), C.addressof(d), out.cell_buffer.data(), out.rec_buffer.data()))
        return out

    def desc(self) -> SceneGridDesc:
        return self._desc

    @property
    def dim(self):
        return tuple(int(v) for v in self._desc.dim)

    def cell_points(self) -> np.ndarray:
        """The cells' scene-point indices as a (dim z, dim y, dim x) array (x fastest), ``GRID_NONE`` where a cell is empty."""
        dx, dy, dz = self.dim
        return self.cell_buffer.to_host().reshape(dz, dy, dx)

    def records(self) -> np.ndarray:
        """The (n_points, 8) records {px, py, pz, 0, nx, ny, nz, 0} the build wrote."""
        return self.rec_buffer.to_host().reshape(-1, 8)

    @property
    def nbytes(self) -> int:
        return self.cell_buffer.size() * 4 + self.rec_buffer.size() * 4


def ICP_Point2Plane(model_pcd: DeviceVector, scene, criteria: ICPConvergenceCriteria = ICPConvergenceCriteria()) -> RegistrationResult:
    """``cuda_icp::ICP_Point2Plane_cuda<Scene>`` (icp.cu:156-223).  Mutates ``model_pcd`` in place."""
    res = np.zeros(1, RESULT)
    d = scene.desc()
    if scene.kind == SCENE_PROJ_CROP:                            # no single-cloud entry point of its own: a batch of one
        off = np.array([0, model_pcd.size() // 3], np.uint32)
        check(_lib.load().pr_icp_batch(model_pcd.data(), ptr(off), 1, scene.kind, C.addressof(d), criteria.c(), ptr(res)))
        return RegistrationResult.from_record(res[0])
    fn = _lib.load().pr_icp_nn if scene.kind == SCENE_NN else _lib.load().pr_icp_grid if scene.kind == SCENE_GRID else _lib.load().pr_icp_proj
    check(fn(model_pcd.data(), model_pcd.size() // 3, C.addressof(d), criteria.c(), ptr(res)))
    return RegistrationResult.from_record(res[0])


class Robust:
    """``pr_robust``: an M-estimator weight on the point-to-plane residual -- ``Robust(ROBUST_HUBER, 0.005)`` -- with the scale ``c`` in metres.
    The descriptor comes from ``pr_robust_describe`` (``inv_c`` is computed there, once, in float32); a bad kind or scale raises."""

    def __init__(self, kind: int, c: float = 0.0):
        self._d = RobustDesc()
        if not 0 <= int(kind) < 2**32:
            raise ValueError(f"kind {kind} is no uint32")
        check(_lib.load().pr_robust_describe(int(kind), float(c), C.addressof(self._d)))

    kind = property(lambda self: int(self._d.kind))
    c = property(lambda self: np.float32(self._d.c))
    inv_c = property(lambda self: np.float32(self._d.inv_c))

    def desc(self) -> RobustDesc:
        return self._d

    def __repr__(self):
        return f"Robust(kind={self.kind}, c={float(self.c)!r})"


def _robust_table(robust, n_levels: int):
    """(pr_robust array, its length) from one ``Robust`` (every level) or a sequence of them (one per level)."""
    rs = [robust] if isinstance(robust, Robust) else list(robust)
    if not rs or not all(isinstance(r, Robust) for r in rs):
        raise ValueError("robust: a Robust or a sequence of them, one per level")
    if len(rs) not in (1, n_levels):
        raise ValueError(f"robust: one descriptor or one per level ({n_levels}), got {len(rs)}")
    return (RobustDesc * len(rs))(*[r.desc() for r in rs]), len(rs)


def ICP_Point2Plane_batch(clouds: DeviceVector, offsets, scene, criteria: ICPConvergenceCriteria = ICPConvergenceCriteria(),
                          robust: Optional[Robust] = None) -> np.ndarray:
    """Many clouds against one scene (one launch per iteration).  offsets: P+1 point offsets.  ``robust``: a ``Robust`` weight
    (``pr_icp_batch_robust``); None is the plain call."""
    offsets = np.ascontiguousarray(offsets, np.uint32)
    if len(offsets) == 0:
        raise ValueError("offsets: P + 1 point offsets (at least one)")
    if int(offsets[-1]) * 3 > clouds.size():
        raise ValueError(f"offsets end at point {int(offsets[-1])}, the cloud buffer holds {clouds.size() // 3}")
    res = np.zeros(len(offsets) - 1, RESULT)
    d = scene.desc()
    if robust is not None:
        check(_lib.load().pr_icp_batch_robust(clouds.data(), ptr(offsets), len(offsets) - 1, scene.kind, C.addressof(d), criteria.c(),
                                              C.addressof(robust.desc()), ptr(res)))
        return res
    check(_lib.load().pr_icp_batch(clouds.data(), ptr(offsets), len(offsets) - 1, scene.kind, C.addressof(d), criteria.c(), ptr(res)))
    return res


def debug_robust_terms(model_pcd: DeviceVector, scene, robust: Robust, update=None, packed: bool = False, want_corr: bool = True):
    """``pr_debug_robust_terms``: ``debug_contrib29`` with the weighted terms of ``robust``.  Returns (terms (n, 29), corr (n, 8) or None):
    corr rows are {dx, dy, dz, valid, nx, ny, nz, w}, zero where the point has no valid correspondence."""
    n = model_pcd.size() // 3
    out = np.zeros((n, 29), np.float32)
    corr = np.zeros((n, 8), np.float32) if want_corr else None
    d = scene.desc()
    u = _f32(update, -1) if update is not None else None
    check(_lib.load().pr_debug_robust_terms(model_pcd.data(), n, scene.kind, C.addressof(d), ptr(u) if u is not None else None, int(packed),
                                            C.addressof(robust.desc()), ptr(out), ptr(corr) if corr is not None else None))
    return out, corr


def debug_contrib29(model_pcd: DeviceVector, scene, update=None, packed: bool = False) -> np.ndarray:
    """``pr_debug_contrib29``: the (n, 29) per-point terms of one correspondence pass; ``update`` (4x4 or None) is applied to the cloud first."""
    n = model_pcd.size() // 3
    out = np.zeros((n, 29), np.float32)
    d = scene.desc()
    u = _f32(update, -1) if update is not None else None
    check(_lib.load().pr_debug_contrib29(model_pcd.data(), n, scene.kind, C.addressof(d), ptr(u) if u is not None else None, int(packed), ptr(out)))
    return out


def debug_pose_iteration(sums, n_points, criteria, iteration: int, on_device: bool, state=None):
    """``pr_debug_pose_iteration``: one ICP iteration (icp.cu:178-212) for every row of ``sums`` (n, 29), on the device (the wavefront
    iteration of the device-solve loop) or on the host (the host-solve loop's).  ``state``: RESULT records as the previous iteration left
    them (default: identity, rmse and fitness 0).  Returns (state after the iteration, updates E (n, 4, 4), finished (n,) bool)."""
    s = _f32(sums, -1).reshape(-1, 29)
    n = len(s)
    cnt = np.ascontiguousarray(n_points, dtype=np.uint32).reshape(-1)
    if len(cnt) != n:
        raise ValueError(f"n_points: one count per row of sums, got {len(cnt)} for {n}")
    st = np.zeros(n, RESULT)
    if state is None:
        st["T"] = np.eye(4, dtype=np.float32).reshape(16)
    else:
        st[:] = np.asarray(state, RESULT).reshape(n)
    upd = np.zeros((n, 16), np.float32)
    fin = np.zeros(n, np.uint32)
    check(_lib.load().pr_debug_pose_iteration(ptr(s), ptr(cnt), n, criteria.c(), int(iteration), int(bool(on_device)), ptr(st), ptr(upd), ptr(fin)))
    return st, upd.reshape(n, 4, 4), fin.astype(bool)


def trace_sums(n_hyp: int, n_passes: int) -> np.ndarray:
    """``pr_debug_trace_sums``: arms the recorder for this thread's next synchronous ICP call (``ICP_Point2Plane[_batch]``, ``refine_batch``
    under host solve) and returns the NaN-prefilled (n_passes, n_hyp, 29) float32 array that call fills: row (it, i) = the 29 sums
    hypothesis i's iteration ``it`` consumed; rows of skipped or finished hypotheses stay NaN.  The array is kept alive here until the
    next ``trace_sums`` / ``trace_sums_off`` of the thread, so dropping the returned reference early is harmless."""
    rows = np.full((int(n_passes), int(n_hyp), 29), np.nan, np.float32)
    _tls.trace_rows = rows
    check(_lib.load().pr_debug_trace_sums(ptr(rows), int(n_hyp), int(n_passes)))
    return rows


def trace_sums_off():
    """Disarms a recorder that no call has consumed yet (``pr_debug_trace_sums(NULL, 0, 0)``)."""
    check(_lib.load().pr_debug_trace_sums(None, 0, 0))
    _tls.trace_rows = None


def debug_nn_records(scene: "Scene_nn", camera=None) -> dict:
    """``pr_debug_nn_records``: the derived search data of a kd-tree scene as numpy arrays -- ``topo`` (n, 4) int32, ``bmin`` / ``bmax`` (n, 4)
    float32, ``rec64`` (n, 16) float32, ``rec32`` (n, 8) uint32, ``desc`` (n, 2) uint32, ``pts`` (points, 4) float32, ``info`` (24,) uint32,
    ``wide`` (info[9], 32) uint32 and, with ``camera`` = (w, h, fx, fy, cx, cy), ``cell_idx`` (h, w) int32 and ``grid`` (cells, 4) float32 --
    plus ``counts`` (the ``pr_nn_records_counts`` fields).  Without a grid ``cell_idx`` and ``grid`` are None."""
    d = scene.desc()
    k = None
    w = h = 0
    if camera is not None:
        w, h = int(camera[0]), int(camera[1])
        k = np.array(camera[2:6], np.float32)
    lib = _lib.load()
    cnt = _lib.NNRecordsCounts()
    check(lib.pr_debug_nn_records(C.addressof(d), w, h, ptr(k) if k is not None else None, C.byref(cnt), None))
    n, m = cnt.n_nodes, cnt.n_points
    arrs = {"topo": np.zeros((n, 4), np.int32), "bmin": np.zeros((n, 4), np.float32), "bmax": np.zeros((n, 4), np.float32),
            "rec64": np.zeros((n, 16), np.float32), "rec32": np.zeros((n, 8), np.uint32), "desc": np.zeros((n, 2), np.uint32),
            "pts": np.zeros((m, 4), np.float32), "info": np.zeros(24, np.uint32), "wide": np.zeros((cnt.n_wide, 32), np.uint32),
            "cell_idx": np.zeros((cnt.grid_h, cnt.grid_w), np.int32) if cnt.grid_w else None,
            "grid": np.zeros((cnt.grid_cells, 4), np.float32) if cnt.grid_w else None}
    out = _lib.NNRecordsOut(*[(ptr(arrs[f]) if arrs[f] is not None and arrs[f].size else None) for f in _lib.NN_RECORDS_FIELDS])
    check(lib.pr_debug_nn_records(C.addressof(d), w, h, ptr(k) if k is not None else None, C.byref(cnt), C.byref(out)))
    arrs["counts"] = {f: int(getattr(cnt, f)) for f, _ in _lib.NNRecordsCounts._fields_}
    return arrs


def refine_batch(tris, poses, width: int, height: int, proj, K, scene,
                 criteria: ICPConvergenceCriteria = ICPConvergenceCriteria(), results_dev: Optional[int] = None,
                 roi: Optional[Sequence[int]] = None, robust: Optional[Robust] = None):
    """Fused hypothesis refinement (test.cpp:143-172 for a batch): render -> cloud -> ICP on the device.
    Returns (records[P] of RESULT dtype or None when results_dev is given, cloud sizes[P]).
    ``roi`` = (x, y, width, height): render only inside the window (renderer.h:199), clouds with tl = (x, y).
    ``robust``: a ``Robust`` weight -- the call runs as a one-level stride-1 ``refine_pyramid`` (``pr_refine_pyramid_robust``)."""
    if robust is not None:
        if results_dev is not None:
            raise ValueError("robust and results_dev together are not offered")
        return refine_pyramid(tris, poses, width, height, proj, K, scene, levels=((1, criteria),), roi=roi, robust=robust)
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    pj, k = _f32(proj, -1), _f32(K, -1)
    sizes = np.zeros(len(poses), np.uint32)
    d = scene.desc()
    if roi is not None:
        if results_dev is not None:
            raise ValueError("roi and results_dev together: use refine_submit")
        res = np.zeros(len(poses), RESULT)
        check(_lib.load().pr_refine_batch_roi(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), ptr(k),
                                              scene.kind, C.addressof(d), criteria.c(), Roi(*roi), ptr(res), ptr(sizes)))
        return res, sizes
    if results_dev is None:
        res = np.zeros(len(poses), RESULT)
        check(_lib.load().pr_refine_batch(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), ptr(k),
                                          scene.kind, C.addressof(d), criteria.c(), ptr(res), ptr(sizes)))
        return res, sizes
    check(_lib.load().pr_refine_batch_dev(td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), ptr(k),
                                          scene.kind, C.addressof(d), criteria.c(), int(results_dev), ptr(sizes)))
    return None, sizes


_tls = threading.local()


def _slots() -> dict:
    """Outputs (and input owners) of the batches in flight, per host thread: a thread with a private context
    (``thread_context``) has slots of its own, and the arrays the library writes into at ``refine_wait`` must stay alive until then."""
    d = getattr(_tls, "inflight", None)
    if d is None:
        d = _tls.inflight = {}
    return d


def refine_submit(slot: int, tris, poses, width: int, height: int, proj, K, scene,
                  criteria: ICPConvergenceCriteria = ICPConvergenceCriteria(), results_dev: Optional[int] = None,
                  roi: Sequence[int] = (0, 0, 0, 0), also_host: bool = False):
    """Asynchronous ``refine_batch``: enqueue the batch on ``slot`` (0 or 1) and return at once; ``refine_wait(slot)``
    delivers what ``refine_batch`` returns.  With two slots, batch k+1 is enqueued while batch k runs.  ``results_dev``: the records go to
    that device block (a sharded job's gather reads them there); ``also_host``: and to the host as well, like the reference's by-value return."""
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    pj, k = _f32(proj, -1), _f32(K, -1)
    sizes = np.zeros(len(poses), np.uint32)
    res = np.zeros(len(poses), RESULT) if (results_dev is None or also_host) else None
    d = scene.desc()
    check(_lib.load().pr_refine_submit_roi(int(slot), td.data(), td.size() // 9, ptr(poses), len(poses), width, height, ptr(pj), ptr(k),
                                           scene.kind, C.addressof(d), criteria.c(), Roi(*roi), ptr(res) if res is not None else None,
                                           int(results_dev) if results_dev is not None else None, ptr(sizes)))
    _slots()[int(slot)] = (res, sizes, td, scene)              # keep the output arrays (and the inputs' owners) alive


def refine_wait(slot: int):
    """Block until the batch submitted on ``slot`` is finished; returns (records or None, cloud sizes)."""
    check(_lib.load().pr_refine_wait(int(slot)))
    res, sizes, _, _ = _slots().pop(int(slot))
    return res, sizes


# ------------------------------------------------------------------------------------------------
# verification: render-and-compare scoring of (refined) hypotheses
# ------------------------------------------------------------------------------------------------
def score_poses(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int,
                roi: Sequence[int] = (0, 0, 0, 0)) -> np.ndarray:
    """``pr_score_poses``: render every pose (inside ``roi`` only, when one is given) and compare it pixel by pixel with the scene
    depth (mm).  ``scene_depth`` is a DeviceVector of ``width * height`` int32 or uint16 values, or a host (height, width) array of
    either dtype, which is uploaded for the call.  Returns SCORE[P]: visible / inlier / occluded / violation / missing pixel counts and
    the exact sum of |r - s| over the inliers."""
    return _score_poses(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, roi)


def refined_poses(records, poses) -> np.ndarray:
    """``pr_refined_poses``: the pose each ICP result stands for, ``T' @ pose`` with the result's translation scaled from metres
    (the clouds) to millimetres (the poses).  float32[P, 4, 4]."""
    rec = np.ascontiguousarray(records, RESULT)
    poses = _f32(poses, (-1, 16))
    if len(rec) != len(poses):
        raise ValueError(f"{len(rec)} results for {len(poses)} poses")
    out = np.zeros((len(poses), 4, 4), np.float32)
    _lib.load().pr_refined_poses(ptr(rec), ptr(poses), len(poses), ptr(out))
    return out


def rank_hypotheses(scores) -> np.ndarray:
    """Hypothesis indices, best first.  The policy: inlier fraction ``inlier / (visible - occluded)`` in float64, descending --
    occluded pixels neither count for nor against a hypothesis, missing and violating ones count against it.  Hypotheses with
    ``visible - occluded == 0`` (nothing rendered, or only occluded pixels) come last.  Ties: more inliers first, then the lower index."""
    sc = np.asarray(scores)
    inl = sc["inlier"].astype(np.int64)
    den = sc["visible"].astype(np.int64) - sc["occluded"].astype(np.int64)
    empty = den <= 0
    frac = np.where(empty, 0.0, inl.astype(np.float64) / np.where(empty, 1, den).astype(np.float64))
    idx = np.arange(len(sc), dtype=np.int64)
    return np.lexsort((idx, -inl, -frac, empty.astype(np.int8))).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# mixed batches: hypotheses of several meshes in one call
# ------------------------------------------------------------------------------------------------
def _mesh_index(mesh_index, n_poses: int, n_meshes: int) -> np.ndarray:
    """``mesh_index`` checked before anything reaches the library: integers, one per pose, each in [0, n_meshes)."""
    a = np.asarray(mesh_index)
    if a.ndim != 1 or len(a) != n_poses:
        raise ValueError(f"mesh_index must hold one entry per pose: got shape {a.shape} for {n_poses} poses")
    if n_poses and a.dtype.kind not in "iu":
        raise ValueError(f"mesh_index must be an integer array, got {a.dtype}")
    if n_poses and (a.min() < 0 or a.max() >= n_meshes):
        raise ValueError(f"mesh_index values must lie in [0, {n_meshes}): got {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a, np.uint32)


def _mesh_table(meshes):
    """(pr_mesh_ref array, device buffers kept alive for the call) from a sequence of what ``render`` / ``refine_batch`` accept as ``tris``."""
    devs = [_tris_dev(m) for m in meshes]
    table = (MeshRef * max(1, len(devs)))(*[MeshRef(d.data() or None, d.size() // 9) for d in devs])
    return table, devs


def _multi_inputs(meshes, mesh_index, poses):
    meshes = list(meshes)
    poses = _f32(poses, (-1, 16))
    idx = _mesh_index(mesh_index, len(poses), len(meshes))
    if not meshes and len(poses):
        raise ValueError("no meshes for the poses")
    table, devs = _mesh_table(meshes)
    return table, devs, idx, poses


def render_multi(meshes, mesh_index, poses, width: int, height: int, proj, roi: Sequence[int] = (0, 0, 0, 0)) -> DeviceVector:
    """``pr_render_multi``: ``render`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; images in pose order."""
    table, devs, idx, poses = _multi_inputs(meshes, mesh_index, poses)
    rw, rh = (roi[2], roi[3]) if roi[2] > 0 and roi[3] > 0 else (width, height)
    out = DeviceVector(len(poses) * rw * rh, np.int32)
    pj = _f32(proj, -1)
    check(_lib.load().pr_render_multi(table, len(devs), ptr(idx), ptr(poses), len(poses), width, height, ptr(pj), Roi(*roi), out.data()))
    return out


def refine_batch_multi(meshes, mesh_index, poses, width: int, height: int, proj, K, scene,
                       criteria: ICPConvergenceCriteria = ICPConvergenceCriteria(), roi: Optional[Sequence[int]] = None,
                       robust: Optional["Robust"] = None):
    """``pr_refine_batch_multi``: ``refine_batch`` for a batch whose pose i uses ``meshes[mesh_index[i]]`` (a ``Model``, a ``DeviceVector``
    or a host triangle array each), in one call.  Returns (records[P], cloud sizes[P]) in pose order, each equal to what ``refine_batch``
    gives that pose with its own mesh.  ``robust``: as for ``refine_batch`` (``pr_refine_pyramid_robust_multi``, one level of stride 1)."""
    if robust is not None:
        return refine_pyramid_multi(meshes, mesh_index, poses, width, height, proj, K, scene, levels=((1, criteria),), roi=roi, robust=robust)
    table, devs, idx, poses = _multi_inputs(meshes, mesh_index, poses)
    pj, k = _f32(proj, -1), _f32(K, -1)
    res = np.zeros(len(poses), RESULT)
    sizes = np.zeros(len(poses), np.uint32)
    d = scene.desc()
    check(_lib.load().pr_refine_batch_multi(table, len(devs), ptr(idx), ptr(poses), len(poses), width, height, ptr(pj), ptr(k), scene.kind,
                                            C.addressof(d), criteria.c(), Roi(*(roi if roi is not None else (0, 0, 0, 0))), ptr(res), ptr(sizes)))
    return res, sizes


# ------------------------------------------------------------------------------------------------
# coarse-to-fine refinement: a pyramid of strided clouds per hypothesis
# ------------------------------------------------------------------------------------------------
def PyramidLevel(stride: int, criteria) -> _PyramidLevel:
    """One level of a schedule (``pr_pyramid_level``): every ``stride``-th frame column and row of the rendered cloud, refined with
    ``criteria`` -- an ``ICPConvergenceCriteria`` or a (relative_fitness, relative_rmse, max_iteration) triple."""
    c = criteria.c() if isinstance(criteria, ICPConvergenceCriteria) else Criteria(float(criteria[0]), float(criteria[1]), int(criteria[2]))
    if not 0 <= int(stride) < 2**32:
        raise ValueError(f"stride {stride} is no uint32")
    return _PyramidLevel(int(stride), c)


PYRAMID_DEFAULT = ((4, (0, 0, 12)), (2, (0, 0, 5)), (1, (0, 0, 3)))
"""The default schedule, coarse first, as (stride, (relative_fitness, relative_rmse, max_iteration)): 12 iterations on every 4th column
and row, 5 on every 2nd, 3 at full resolution.  Measured with the CPU oracle on ``synth.hypotheses(48)`` (obj_06 scenario, projective
scene, canonical sums, 2048 points per block) against 20 full-resolution iterations: 0.301 of the point-passes; for all 43 hypotheses
that converge (fitness >= 0.9) the final translation differs by at most 0.016 mm and fitness / rmse agree to the 4th digit; the other five
converge under neither schedule.  Over ``synth.hypotheses(256)`` the same comparison loses 2 of the 218 hypotheses the full run converges on
(the coarse level walks them into another basin) and keeps 212 within 0.05 mm: a schedule is a trade, and no policy for choosing one is
part of this module.  What it costs or saves on an MI355X -- a third less time on a kd-tree scene, nothing on a projective one -- is in
profiles/pyramid/README.md."""


def _level_table(levels):
    lv = [l if isinstance(l, _PyramidLevel) else PyramidLevel(*l) for l in levels]
    return (_PyramidLevel * max(1, len(lv)))(*lv), len(lv)


def _pyramid_outputs(n_levels: int, n_poses: int, levels, return_levels: bool, res, lres, lsizes):
    if return_levels:
        return res, lres, lsizes
    # the stride-1 cloud size when a level has stride 1 (what refine_batch returns), else the LAST level's cloud size
    strides = [l.stride for l in levels[:n_levels]]
    row = strides.index(1) if 1 in strides else n_levels - 1
    return res, lsizes[row].copy()


def refine_pyramid(tris, poses, width: int, height: int, proj, K, scene, levels=PYRAMID_DEFAULT, roi: Optional[Sequence[int]] = None,
                   return_levels: bool = False, robust=None):
    """``pr_refine_pyramid``: ``refine_batch`` run coarse to fine.  ``levels``: 1..4 ``PyramidLevel`` (or (stride, criteria) pairs), coarse
    first; level l refines the cloud of every ``stride``-th FRAME column and row, moved by what the levels before it found.  Returns
    (records[P], sizes[P]): the accumulated transform with the last level's fitness and rmse, and the stride-1 cloud size as ``refine_batch``
    returns it when a level has stride 1 -- otherwise the last level's cloud size.  ``return_levels=True``: (records[P],
    level_records[L, P], level_sizes[L, P]).  One level of stride 1 equals ``refine_batch`` byte for byte.  ``robust``: one ``Robust`` for
    every level or one per level (``pr_refine_pyramid_robust``); None is the plain call."""
    table, n_levels = _level_table(levels)
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    pj, k = _f32(proj, -1), _f32(K, -1)
    P = len(poses)
    res = np.zeros(P, RESULT)
    lres = np.zeros((max(1, n_levels), P), RESULT)
    lsizes = np.zeros((max(1, n_levels), P), np.uint32)
    d = scene.desc()
    if robust is not None:
        rtable, n_robust = _robust_table(robust, n_levels)
        check(_lib.load().pr_refine_pyramid_robust(td.data() or None, td.size() // 9, ptr(poses), P, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                                   table, n_levels, Roi(*(roi if roi is not None else (0, 0, 0, 0))), ptr(res), ptr(lres), ptr(lsizes),
                                                   rtable, n_robust))
        return _pyramid_outputs(n_levels, P, table, return_levels, res, lres, lsizes)
    check(_lib.load().pr_refine_pyramid(td.data() or None, td.size() // 9, ptr(poses), P, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                        table, n_levels, Roi(*(roi if roi is not None else (0, 0, 0, 0))), ptr(res), ptr(lres), ptr(lsizes)))
    return _pyramid_outputs(n_levels, P, table, return_levels, res, lres, lsizes)


def refine_pyramid_multi(meshes, mesh_index, poses, width: int, height: int, proj, K, scene, levels=PYRAMID_DEFAULT,
                         roi: Optional[Sequence[int]] = None, return_levels: bool = False, robust=None):
    """``pr_refine_pyramid_multi``: ``refine_pyramid`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; every output in pose
    order and equal to what ``refine_pyramid`` gives that pose with its own mesh.  ``robust``: as for ``refine_pyramid``."""
    table, n_levels = _level_table(levels)
    mtable, devs, idx, poses = _multi_inputs(meshes, mesh_index, poses)
    pj, k = _f32(proj, -1), _f32(K, -1)
    P = len(poses)
    res = np.zeros(P, RESULT)
    lres = np.zeros((max(1, n_levels), P), RESULT)
    lsizes = np.zeros((max(1, n_levels), P), np.uint32)
    d = scene.desc()
    if robust is not None:
        rtable, n_robust = _robust_table(robust, n_levels)
        check(_lib.load().pr_refine_pyramid_robust_multi(mtable, len(devs), ptr(idx), ptr(poses), P, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                                         table, n_levels, Roi(*(roi if roi is not None else (0, 0, 0, 0))), ptr(res), ptr(lres), ptr(lsizes),
                                                         rtable, n_robust))
        return _pyramid_outputs(n_levels, P, table, return_levels, res, lres, lsizes)
    check(_lib.load().pr_refine_pyramid_multi(mtable, len(devs), ptr(idx), ptr(poses), P, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                              table, n_levels, Roi(*(roi if roi is not None else (0, 0, 0, 0))), ptr(res), ptr(lres), ptr(lsizes)))
    return _pyramid_outputs(n_levels, P, table, return_levels, res, lres, lsizes)


def _scene_depth_dev(scene_depth, width: int, height: int) -> DeviceVector:
    if isinstance(scene_depth, DeviceVector):
        sd = scene_depth
    else:
        arr = np.ascontiguousarray(scene_depth)
        if arr.dtype not in (np.uint16, np.int32):
            raise ValueError("scene depth must be CV_16U or CV_32S")
        sd = DeviceVector.from_host(arr.reshape(-1))
    if sd.dtype not in (np.uint16, np.int32):
        raise ValueError("scene depth must be CV_16U or CV_32S")
    if sd.size() != width * height:
        raise ValueError(f"scene depth holds {sd.size()} values, expected {width} x {height}")
    return sd


# The scoring calls come as pairs, one mesh or a mixed batch, that differ in their leading C arguments only.  A "mesh" below is what
# _one_mesh / _mesh_batch return: (suffix of the entry point's name, its leading arguments, the poses as float32[P, 16], what those point into).
def _one_mesh(tris, poses):
    td = _tris_dev(tris)
    return "", (td.data(), td.size() // 9), _f32(poses, (-1, 16)), td


def _mesh_batch(meshes, mesh_index, poses):
    table, devs, idx, poses = _multi_inputs(meshes, mesh_index, poses)
    return "_multi", (table, len(devs), ptr(idx)), poses, (devs, idx)


def _score_call(name: str, mesh, width: int, height: int, proj, scene_depth, tau_mm: int, roi):
    """(``name`` or ``name_multi`` with the arguments every scoring entry point shares bound -- the caller adds those of its kind --, the number of poses)"""
    suffix, lead, poses, alive = mesh
    pj = _f32(proj, -1)
    sd = _scene_depth_dev(scene_depth, width, height)
    fn = getattr(_lib.load(), name + suffix)

    def call(*outputs, _alive=(alive, poses, pj, sd)):
        check(fn(*lead, ptr(poses), len(poses), width, height, ptr(pj), Roi(*roi), sd.data(), int(sd.dtype == np.int32), int(tau_mm), *outputs))
    return call, len(poses)


def _score_poses(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, roi) -> np.ndarray:
    call, n = _score_call("pr_score_poses", mesh, width, height, proj, scene_depth, tau_mm, roi)
    out = np.zeros(n, SCORE)
    call(ptr(out))
    return out


def score_poses_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int,
                      roi: Sequence[int] = (0, 0, 0, 0)) -> np.ndarray:
    """``pr_score_poses_multi``: ``score_poses`` for a batch whose pose i uses ``meshes[mesh_index[i]]``.  SCORE[P] in pose order."""
    return _score_poses(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, roi)


# ------------------------------------------------------------------------------------------------
# detections: which hypotheses explain the same scene pixels, and a conflict-free choice among them
# ------------------------------------------------------------------------------------------------
OVERLAP_MAX_POSES = 4096                # PR_OVERLAP_MAX_POSES


def _score_overlap(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, roi):
    call, n = _score_call("pr_score_overlap", mesh, width, height, proj, scene_depth, tau_mm, roi)
    out, ov = np.zeros(n, SCORE), np.zeros((n, n), np.uint32)
    call(ptr(out), ptr(ov))
    return out, ov


def score_overlap(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_score_overlap``: ``score_poses`` plus the matrix of shared inlier pixels.  Returns (SCORE[P], uint32[P, P]): the records are
    ``score_poses``' bytes, ``overlap[i, j]`` counts the frame pixels that are inliers of both i and j (symmetric; the diagonal is
    ``scores["inlier"]``).  At most ``OVERLAP_MAX_POSES`` hypotheses per call."""
    return _score_overlap(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, roi)


def score_overlap_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int,
                        roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_score_overlap_multi``: ``score_overlap`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; hypotheses of different
    meshes are compared like any other pair.  (SCORE[P], uint32[P, P]) in pose order."""
    return _score_overlap(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, roi)


def select_greedy(order, overlap, shared_num: int, shared_den: int) -> np.ndarray:
    """``pr_select_greedy`` (host only): walk ``order`` (indices, best first); skip i when ``overlap[i, i] == 0``; accept i unless an
    accepted j has ``overlap[i, j] * shared_den > shared_num * min(overlap[i, i], overlap[j, j])``.  Accepted indices in that order."""
    ov = np.ascontiguousarray(overlap, np.uint32)
    if ov.ndim != 2 or ov.shape[0] != ov.shape[1]:
        raise ValueError(f"overlap must be a square matrix, got shape {ov.shape}")
    od = np.asarray(order)
    if od.ndim != 1 or (len(od) and (od.dtype.kind not in "iu" or od.min() < 0 or od.max() > 0xffffffff)):
        raise ValueError("order must be a 1-d array of non-negative integers")
    if not 0 <= int(shared_num) <= 0xffffffff or not 0 <= int(shared_den) <= 0xffffffff:
        raise ValueError("shared_num and shared_den must fit 32 unsigned bits")
    od = np.ascontiguousarray(od, np.uint32)
    sel = np.zeros(max(1, len(od)), np.uint32)
    n = C.c_uint32(0)
    check(_lib.load().pr_select_greedy(ptr(od), len(od), ptr(ov), len(ov), int(shared_num), int(shared_den), ptr(sel), C.byref(n)))
    return sel[:n.value].astype(np.int64)


def select_hypotheses(scores, overlap, max_shared: Sequence[int] = (1, 4), min_fraction: float = 0.0, order=None) -> np.ndarray:
    """Detections from a scored batch: indices of the hypotheses that survive, best first.  ``order`` defaults to
    ``rank_hypotheses(scores)``, the one definition of "better".  Hypotheses whose rank fraction ``inlier / (visible - occluded)`` is below
    ``min_fraction`` leave ``order`` first; the rest go through ``select_greedy``: a hypothesis is dropped when it shares more than
    ``max_shared = (num, den)`` of the smaller of the two supports with a better one already accepted.  The same call serves a mixed
    batch: conflicts between meshes are resolved by the one global order."""
    sc = np.asarray(scores)
    order = rank_hypotheses(sc) if order is None else np.asarray(order, np.int64)
    den = sc["visible"].astype(np.int64) - sc["occluded"].astype(np.int64)
    frac = np.where(den <= 0, 0.0, sc["inlier"].astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))
    order = order[frac[order] >= float(min_fraction)]
    return select_greedy(order, overlap, int(max_shared[0]), int(max_shared[1]))


# ------------------------------------------------------------------------------------------------
# detections that can coexist: the depth intervals two hypotheses share, pixel by pixel, and a choice among them
# ------------------------------------------------------------------------------------------------
def _pose_penetration(mesh, width: int, height: int, proj, slack_mm: int) -> np.ndarray:
    suffix, lead, poses, alive = mesh
    pj = _f32(proj, -1)
    out = np.zeros((len(poses), len(poses)), PAIR_SOLID)
    check(getattr(_lib.load(), "pr_pose_penetration" + suffix)(*lead, ptr(poses), len(poses), width, height, ptr(pj), int(slack_mm), ptr(out)))
    return out


def pose_penetration(tris, poses, width: int, height: int, proj, slack_mm: int = 0) -> np.ndarray:
    """``pr_pose_penetration``: PAIR_SOLID[P, P].  ``both`` counts the frame pixels two hypotheses both render, ``inter`` those where their
    depth intervals [near, far] overlap by more than ``slack_mm``, ``sum_mm`` / ``max_mm`` the sum and the largest of those overlaps in mm.
    Symmetric; the diagonal is a hypothesis' own thickness (its volume).  At most ``PENETRATION_MAX_POSES`` hypotheses per call."""
    return _pose_penetration(_one_mesh(tris, poses), width, height, proj, slack_mm)


def pose_penetration_multi(meshes, mesh_index, poses, width: int, height: int, proj, slack_mm: int = 0) -> np.ndarray:
    """``pr_pose_penetration_multi``: ``pose_penetration`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; rows and columns in pose order."""
    return _pose_penetration(_mesh_batch(meshes, mesh_index, poses), width, height, proj, slack_mm)


def penetration_fraction(pairs) -> np.ndarray:
    """``sum_mm[i, j] / min(sum_mm[i, i], sum_mm[j, j])`` as float64[P, P]: the share of the smaller volume two hypotheses have in common;
    0 where the smaller volume is 0."""
    s = np.asarray(pairs)["sum_mm"]
    d = np.diag(s)
    lim = np.minimum(d[:, None], d[None, :])
    return np.where(lim == 0, 0.0, s.astype(np.float64) / np.where(lim == 0, 1, lim).astype(np.float64))


def select_disjoint(order, pairs, max_fraction: Sequence[int] = (1, 10)) -> np.ndarray:
    """``pr_select_disjoint`` (host only): walk ``order`` (indices, best first); keep i unless a kept j shares more than
    ``max_fraction = (num, den)`` of the smaller of the two volumes with it.  Kept indices in that order."""
    pr = np.ascontiguousarray(pairs, PAIR_SOLID)
    if pr.ndim != 2 or pr.shape[0] != pr.shape[1]:
        raise ValueError(f"pairs must be a square matrix, got shape {pr.shape}")
    od = np.asarray(order)
    if od.ndim != 1 or (len(od) and (od.dtype.kind not in "iu" or od.min() < 0 or od.max() > 0xffffffff)):
        raise ValueError("order must be a 1-d array of non-negative integers")
    num, den = int(max_fraction[0]), int(max_fraction[1])
    if not 0 <= num <= 0xffffffff or not 0 <= den <= 0xffffffff:
        raise ValueError("max_fraction must be two integers that fit 32 unsigned bits")
    od = np.ascontiguousarray(od, np.uint32)
    sel = np.zeros(max(1, len(od)), np.uint32)
    n = C.c_uint32(0)
    check(_lib.load().pr_select_disjoint(ptr(od), len(od), ptr(pr), len(pr), num, den, ptr(sel), C.byref(n)))
    return sel[:n.value].astype(np.int64)


# ------------------------------------------------------------------------------------------------
# detections by cumulative cover: keep a hypothesis for the inlier pixels it adds to what the better ones already claim
# ------------------------------------------------------------------------------------------------
def _cover_rule(order, n_poses: int, min_new_fraction, min_new: int, max_keep):
    od = np.asarray(order)
    if od.ndim != 1 or (len(od) and (od.dtype.kind not in "iu" or od.min() < 0 or od.max() > 0xffffffff)):
        raise ValueError("order must be a 1-d array of non-negative integers")
    num, den = int(min_new_fraction[0]), int(min_new_fraction[1])
    keep = 0xffffffff if max_keep is None else int(max_keep)
    if not all(0 <= v <= 0xffffffff for v in (num, den, int(min_new), keep)):
        raise ValueError("min_new_fraction, min_new and max_keep must fit 32 unsigned bits")
    return np.ascontiguousarray(od, np.uint32), (num, den, int(min_new), keep)


def _score_cover(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, order, min_new_fraction, min_new: int, max_keep, roi):
    call, n = _score_call("pr_score_cover", mesh, width, height, proj, scene_depth, tau_mm, roi)
    od, rule = _cover_rule(order, n, min_new_fraction, min_new, max_keep)
    out, cov, frame = np.zeros(n, SCORE), np.zeros(n, COVER), np.zeros(1, COVER_FRAME)
    sel = np.zeros(max(1, len(od)), np.uint32)
    ns = C.c_uint32(0)
    call(ptr(od), len(od), *rule, ptr(out), ptr(cov), ptr(frame), ptr(sel), C.byref(ns))
    return out, cov, frame[0], sel[:ns.value].astype(np.int64)


def score_cover(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, order, min_new_fraction: Sequence[int] = (1, 2),
                min_new: int = 1, max_keep: Optional[int] = None, roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_score_cover``: ``score_poses`` plus the cover walk on the device.  ``order`` (indices, best first) is walked with a claimed
    pixel set; a hypothesis with support is accepted while fewer than ``max_keep`` are, when the part of its support that is not claimed
    yet, ``fresh``, is at least ``min_new`` pixels and at least ``min_new_fraction = (num, den)`` of the support; its support is then
    claimed.  Returns (SCORE[P], COVER[P], one COVER_FRAME record, selected indices in acceptance order)."""
    return _score_cover(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, order, min_new_fraction, min_new, max_keep, roi)


def score_cover_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int, order,
                      min_new_fraction: Sequence[int] = (1, 2), min_new: int = 1, max_keep: Optional[int] = None, roi: Sequence[int] = (0, 0, 0, 0)):
    """``pr_score_cover_multi``: ``score_cover`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; hypotheses of different meshes
    claim pixels like any others.  Everything in pose order."""
    return _score_cover(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, order, min_new_fraction, min_new, max_keep, roi)


def _cover_planes(supports) -> np.ndarray:
    """uint64[P, words]: one bit per pixel.  ``supports``: a boolean array whose first axis is the hypothesis, or a sequence of boolean masks of one shape."""
    m = np.asarray(supports)
    if m.dtype != np.bool_ or m.ndim < 1:
        raise ValueError("supports must be boolean masks, one per hypothesis")
    m = m.reshape(len(m), int(np.prod(m.shape[1:])))
    pad = -m.shape[1] % 64
    bits = np.packbits(np.pad(m, ((0, 0), (0, pad))), axis=1, bitorder="little")
    return np.ascontiguousarray(bits).view(np.uint64).reshape(len(m), (m.shape[1] + pad) // 64)


def select_cover_host(supports, order, min_new_fraction: Sequence[int] = (1, 2), min_new: int = 1, max_keep: Optional[int] = None):
    """``pr_select_cover_host`` (host only): the cover rule of ``score_cover`` on supports the caller brings -- boolean masks, one per
    hypothesis (packed to bit planes here), or uint64[P, words] planes.  Returns (COVER[P], one COVER_FRAME record, selected indices)."""
    planes = np.ascontiguousarray(supports) if getattr(supports, "dtype", None) == np.uint64 and np.ndim(supports) == 2 else _cover_planes(supports)
    n = len(planes)
    od, rule = _cover_rule(order, n, min_new_fraction, min_new, max_keep)
    cov, frame = np.zeros(n, COVER), np.zeros(1, COVER_FRAME)
    sel = np.zeros(max(1, len(od)), np.uint32)
    ns = C.c_uint32(0)
    check(_lib.load().pr_select_cover_host(ptr(planes), n, planes.shape[1] if n else 0, ptr(od), len(od), *rule, ptr(cov), ptr(frame), ptr(sel), C.byref(ns)))
    return cov, frame[0], sel[:ns.value].astype(np.int64)


def select_cover(scores, tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, min_new_fraction: Sequence[int] = (1, 2),
                 min_new: int = 1, min_fraction: float = 0.0, order=None, max_keep: Optional[int] = None, roi: Sequence[int] = (0, 0, 0, 0),
                 mesh_index=None):
    """Detections from a scored batch by the cover rule, on the device: ``order`` defaults to ``rank_hypotheses(scores)`` and hypotheses
    whose rank fraction ``inlier / (visible - occluded)`` is below ``min_fraction`` leave it first, exactly as in ``select_hypotheses``;
    the rest are walked by ``score_cover`` (``score_cover_multi`` with ``tris`` a list of meshes when ``mesh_index`` is given).
    ``scores`` are the batch's records from any earlier scoring call.  Returns (selected indices best first, COVER[P], COVER_FRAME record)."""
    sc = np.asarray(scores)
    order = rank_hypotheses(sc) if order is None else np.asarray(order, np.int64)
    den = sc["visible"].astype(np.int64) - sc["occluded"].astype(np.int64)
    frac = np.where(den <= 0, 0.0, sc["inlier"].astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))
    order = order[frac[order] >= float(min_fraction)]
    mesh = _one_mesh(tris, poses) if mesh_index is None else _mesh_batch(tris, mesh_index, poses)
    _, cov, frame, sel = _score_cover(mesh, width, height, proj, scene_depth, tau_mm, order, min_new_fraction, min_new, max_keep, roi)
    return sel, cov, frame


# ------------------------------------------------------------------------------------------------
# visible surface discrepancy (VSD): an estimate and the truth rendered, masked by the scene depth, compared pixel by pixel
# ------------------------------------------------------------------------------------------------
VSD_DELTA_BOP = 15.0                                                  # mm: BOP's visibility tolerance
VSD_TAUS_BOP = tuple(round(0.05 * k, 2) for k in range(1, 11))       # misalignment tolerances as fractions of the model diameter: the caller multiplies
VSD_THRESHOLDS_BOP = tuple(round(0.05 * k, 2) for k in range(1, 11))  # correctness thresholds on the error


def _pose_vsd(mesh_of, est, gt, width: int, height: int, proj, scene_depth, K, delta_mm: float, taus_mm) -> np.ndarray:
    gt = _poses44(gt, "gt").reshape(-1, 16)                           # (what needs no device is checked first)
    taus = _f32(taus_mm, -1)
    k = None if K is None else _f32(K, -1)
    if k is not None and k.size != 9:
        raise ValueError("K must hold 9 values")
    suffix, lead, est, alive = mesh_of(est)
    pj = _f32(proj, -1)
    sd = _scene_depth_dev(scene_depth, width, height)
    out = np.zeros(len(est), VSD)
    check(getattr(_lib.load(), "pr_pose_vsd" + suffix)(*lead, ptr(est), len(est), ptr(gt), len(gt), width, height, ptr(pj), sd.data(), int(sd.dtype == np.int32),
                                                       None if k is None else ptr(k), float(delta_mm), ptr(taus) if len(taus) else None, len(taus), ptr(out)))
    return out


def pose_vsd(tris, est, gt, width: int, height: int, proj, scene_depth, K=None, delta_mm: float = VSD_DELTA_BOP, taus_mm=()) -> np.ndarray:
    """``pr_pose_vsd``: VSD[n] comparing the render of ``est[i]`` with that of ``gt[i]`` -- or of the one pose ``gt`` of shape (4, 4) /
    (1, 4, 4) -- where each is visible in ``scene_depth`` (as ``score_poses`` takes it: a DeviceVector or a host array, int32 or uint16, mm).
    ``K``: 9 intrinsics (distances along the ray), or None (depths).  ``taus_mm``: up to ``VSD_MAX_TAUS`` non-decreasing tolerances in mm.
    Read the records with ``vsd_errors``."""
    return _pose_vsd(lambda e: _one_mesh(tris, e), est, gt, width, height, proj, scene_depth, K, delta_mm, taus_mm)


def pose_vsd_multi(meshes, mesh_index, est, gt, width: int, height: int, proj, scene_depth, K=None, delta_mm: float = VSD_DELTA_BOP,
                   taus_mm=()) -> np.ndarray:
    """``pr_pose_vsd_multi``: ``pose_vsd`` for pairs whose pair i uses ``meshes[mesh_index[i]]``; as many truths as estimates.  VSD[n] in pair order."""
    return _pose_vsd(lambda e: _mesh_batch(meshes, mesh_index, e), est, gt, width, height, proj, scene_depth, K, delta_mm, taus_mm)


def vsd_errors(records, n_taus: int) -> np.ndarray:
    """BOP's VSD error of every record for its first ``n_taus`` tolerances, float64[n, n_taus]: ``(far[k] + uni - inter) / uni``, 1 where ``uni == 0``."""
    r = np.asarray(records)
    if not 0 <= int(n_taus) <= VSD_MAX_TAUS:
        raise ValueError(f"n_taus must lie in 0 .. {VSD_MAX_TAUS}")
    uni, inter = r["uni"].astype(np.float64)[..., None], r["inter"].astype(np.float64)[..., None]
    far = r["far"][..., :int(n_taus)].astype(np.float64)
    return np.where(uni > 0, (far + uni - inter) / np.where(uni > 0, uni, 1.0), 1.0)


def vsd_recall(errors, thresholds=VSD_THRESHOLDS_BOP) -> float:
    """The fraction of (pose, tau, threshold) triples with ``error < threshold``: BOP's average recall over the taus of ``errors`` and ``thresholds``."""
    e = np.asarray(errors, np.float64)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    if e.size == 0 or th.size == 0:
        return 0.0
    return float((e[..., None] < th).mean())


# ------------------------------------------------------------------------------------------------
# pose distances: how far apart are two poses (ADD / MSSD / MSPD over a symmetry set), duplicates in pose space
# ------------------------------------------------------------------------------------------------
def _points_dev(points) -> DeviceVector:
    if isinstance(points, Model):
        return points.device_vertices()
    if isinstance(points, DeviceVector):
        return points
    return DeviceVector.from_host(_f32(points, -1))


def _poses44(p, name: str) -> np.ndarray:
    a = _f32(p)
    if a.size % 16 or (a.ndim >= 2 and a.shape[-2:] != (4, 4) and a.shape[-1] != 16):
        raise ValueError(f"{name} must hold 4x4 matrices, got shape {a.shape}")
    return a.reshape(-1, 4, 4)


def _pose_distance(points, a: np.ndarray, b: np.ndarray, all_pairs: bool, syms, K) -> np.ndarray:
    pd = _points_dev(points)
    if pd.size() % 3:
        raise ValueError("points must hold 3 float32 per point")
    sy = np.zeros((0, 4, 4), np.float32) if syms is None else _poses44(syms, "syms")
    k = None if K is None else _f32(K, -1)
    if k is not None and k.size != 9:
        raise ValueError("K must hold 9 values")
    out = np.zeros(len(a) * len(b) if all_pairs else len(a), POSE_DIST)
    check(_lib.load().pr_pose_distance(pd.data() or None, pd.size() // 3, ptr(a), len(a), ptr(b), len(b), int(all_pairs), ptr(sy) if len(sy) else None,
                                       len(sy), None if k is None else ptr(k), ptr(out)))
    return out


def pose_distance(points, a, b, syms=None, K=None) -> np.ndarray:
    """``pr_pose_distance``, pair by pair: POSE_DIST[n] comparing ``a[i]`` with ``b[i]`` -- or every ``a[i]`` with the one pose ``b`` of
    shape (4, 4) / (1, 4, 4) ("everything against one ground truth").  ``points``: a ``Model`` (its ``device_vertices()``), a DeviceVector of
    3 float32 per point, or a host (n, 3) array, uploaded for the call.  Poses in mm; ``syms``: up to ``POSE_DIST_MAX_SYMS`` 4x4 symmetry
    transforms of the model (None: the identity); ``K``: 9 intrinsics, or None for no image-space distance.  Read the records with
    ``mean_displacement`` (ADD), ``max_displacement`` (MSSD) and ``max_projection`` (MSPD)."""
    a, b = _poses44(a, "a"), _poses44(b, "b")
    if len(b) == 1 and len(a) != 1:
        return _pose_distance(points, a, b, True, syms, K)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} poses against {len(b)}: pair mode takes as many of each (or one b)")
    return _pose_distance(points, a, b, False, syms, K)


def pose_distance_matrix(points, a, b=None, syms=None, K=None) -> np.ndarray:
    """``pr_pose_distance`` with ``all_pairs``: POSE_DIST[n_a, n_b], entry [i, j] comparing ``a[i]`` with ``b[j]``; ``b=None`` means ``a``
    (the matrix ``merge_duplicates`` takes).  At most ``POSE_DIST_MAX_POSES`` poses a side.  Arguments as for ``pose_distance``."""
    a = _poses44(a, "a")
    b = a if b is None else _poses44(b, "b")
    return _pose_distance(points, a, b, True, syms, K).reshape(len(a), len(b))


def mean_displacement(d) -> np.ndarray:
    """ADD in mm, float64: ``disp_sum_q16 / 65536 / n_points``."""
    d = np.asarray(d)
    return d["disp_sum_q16"].astype(np.float64) / 65536.0 / d["n_points"].astype(np.float64)


def max_displacement(d) -> np.ndarray:
    """MSSD in mm, float64: the square root of ``max_disp_sq``."""
    return np.sqrt(np.asarray(d)["max_disp_sq"].astype(np.float64))


def max_projection(d) -> np.ndarray:
    """MSPD in pixels, float64: the square root of ``max_proj_sq`` (inf where a pose puts a point at Z <= 0; 0 when no K was given)."""
    return np.sqrt(np.asarray(d)["max_proj_sq"].astype(np.float64))


def symmetry_rotations(axis, n: int, center=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The ``n`` transforms of an n-fold rotational symmetry, float32[n, 4, 4]: rotation by 2 pi k / n about the line through ``center``
    along ``axis``, the identity first.  Computed in float64 (Rodrigues' formula) and rounded once."""
    n = int(n)
    ax = np.asarray(axis, np.float64).reshape(3)
    norm = np.linalg.norm(ax)
    if n < 1 or not np.isfinite(norm) or norm == 0.0:
        raise ValueError("symmetry_rotations: n >= 1 and a non-zero axis")
    ax = ax / norm
    c0 = np.asarray(center, np.float64).reshape(3)
    kx = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    out = np.zeros((n, 4, 4), np.float64)
    for k in range(n):
        ang = 2.0 * np.pi * k / n
        r = np.eye(3) if k == 0 else np.eye(3) + np.sin(ang) * kx + (1.0 - np.cos(ang)) * (kx @ kx)
        out[k, :3, :3] = r
        out[k, :3, 3] = c0 - r @ c0
        out[k, 3, 3] = 1.0
    return out.astype(np.float32)


def merge_duplicates(order, dist, max_disp_mm: float):
    """``pr_cluster_greedy`` (host only): walk ``order`` (indices, best first) and keep i unless an already kept j lies within
    ``max_disp_mm`` of it by ``max_disp_sq``, asked in both directions of ``dist`` (the POSE_DIST[P, P] of ``pose_distance_matrix(points, poses)``).
    Returns (kept, representative): the kept indices in that order, and int64[P] with, for every i of ``order``, the kept hypothesis
    that absorbed it (itself if kept); -1 for hypotheses outside ``order``."""
    dm = np.ascontiguousarray(dist, POSE_DIST)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError(f"dist must be a square matrix, got shape {dm.shape}")
    od = np.asarray(order)
    if od.ndim != 1 or (len(od) and (od.dtype.kind not in "iu" or od.min() < 0 or od.max() > 0xffffffff)):
        raise ValueError("order must be a 1-d array of non-negative integers")
    od = np.ascontiguousarray(od, np.uint32)
    kept = np.zeros(max(1, len(od)), np.uint32)
    rep = np.full(max(1, len(dm)), 0xffffffff, np.uint32)
    n = C.c_uint32(0)
    check(_lib.load().pr_cluster_greedy(ptr(od), len(od), ptr(dm), len(dm), float(max_disp_mm), ptr(kept), C.byref(n), ptr(rep)))
    rep = rep[:len(dm)].astype(np.int64)
    rep[rep == 0xffffffff] = -1
    return kept[:n.value].astype(np.int64), rep


# ------------------------------------------------------------------------------------------------
# hypotheses from the scene: point-pair-feature voting (pr_ppf_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def ppf_describe(diameter_mm: float, dist_step_mm: float, n_angle: int = 15, n_alpha: int = 30, flip_model_normals: bool = False) -> PPFParams:
    """``pr_ppf_describe`` (host only): the descriptor with its bin-edge and bin-centre tables."""
    pp = PPFParams()
    check(_lib.load().pr_ppf_describe(float(diameter_mm), float(dist_step_mm), int(n_angle), int(n_alpha), int(bool(flip_model_normals)), C.addressof(pp)))
    return pp


def ppf_model_sample(tris, step_mm: float, flip_normals: bool = False):
    """``pr_ppf_model_sample`` (host only): (points float32[n, 3], normals float32[n, 3]) of a mesh at spacing ``step_mm``: one lattice point per
    occupied voxel.  More than ``PPF_MAX_MODEL_POINTS`` raises PoseRefineError(PR_ERR_INVALID): coarsen the step."""
    t = _f32(tris.tris if isinstance(tris, Model) else tris, (-1, 3, 3))
    pts = np.zeros((PPF_MAX_MODEL_POINTS, 3), np.float32)
    nrm = np.zeros((PPF_MAX_MODEL_POINTS, 3), np.float32)
    n = C.c_uint32(0)
    check(_lib.load().pr_ppf_model_sample(ptr(t) if len(t) else None, len(t), float(step_mm), int(bool(flip_normals)), ptr(pts), ptr(nrm), C.byref(n)))
    return pts[:n.value].copy(), nrm[:n.value].copy()


def ppf_peak_pose(params: PPFParams, model_point, model_normal, scene_point, scene_normal, alpha_bin: int) -> np.ndarray:
    """``pr_ppf_peak_pose`` (host only): the float32 4x4 pose of one peak."""
    a = [_f32(v, 3) for v in (model_point, model_normal, scene_point, scene_normal)]
    out = np.zeros((4, 4), np.float32)
    check(_lib.load().pr_ppf_peak_pose(C.addressof(params), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), int(alpha_bin), ptr(out)))
    return out


class PPFModel:
    """The point-pair-feature model of one mesh: its oriented sample points (host, made on construction -- no device needed) and, on the device
    from the first use on, the direct-addressed pair table of ``pr_ppf_model_build_dev``.  ``step_mm`` defaults to 0.05 of the diameter (the
    diagonal of the vertices' box), ``dist_step_mm`` to ``step_mm``.  ``flip_normals=False`` is right for meshes wound like obj_06, whose
    face normals point outwards: the scene's normals point towards the camera, and so does the outward normal of a visible face."""

    def __init__(self, tris, step_mm: Optional[float] = None, n_angle: int = 15, n_alpha: int = 30, dist_step_mm: Optional[float] = None,
                 flip_normals: bool = False):
        t = _f32(tris.tris if isinstance(tris, Model) else tris, (-1, 3, 3))
        v = t.reshape(-1, 3).astype(np.float64)
        self.diameter = float(np.float32(np.linalg.norm(v.max(0) - v.min(0)))) if len(v) else 0.0
        self.step_mm = float(np.float32(0.05 * self.diameter if step_mm is None else step_mm))
        self.dist_step_mm = float(np.float32(self.step_mm if dist_step_mm is None else dist_step_mm))
        self.params = ppf_describe(self.diameter, self.dist_step_mm, n_angle, n_alpha, flip_normals)
        self.points, self.normals = ppf_model_sample(t, self.step_mm, flip_normals)
        if len(self.points) == 0:
            raise ValueError("PPFModel: the mesh has no sample points")
        if len(self.points) * n_alpha > PPF_MAX_CELLS:
            raise ValueError(f"PPFModel: {len(self.points)} points x {n_alpha} alpha bins exceed PPF_MAX_CELLS = {PPF_MAX_CELLS}: coarsen step_mm")
        self._points_dev = self._normals_dev = self.offsets = self.entries = None
        self.n_entries = 0

    def device_points(self) -> DeviceVector:
        """The sample points on the device (3 float32 each): also the points ``generate_hypotheses`` merges duplicates over."""
        if self._points_dev is None:
            self._points_dev = DeviceVector.from_host(self.points.reshape(-1))
            self._normals_dev = DeviceVector.from_host(self.normals.reshape(-1))
        return self._points_dev

    def build(self) -> "PPFModel":
        """``pr_ppf_model_build_dev``, once: ``offsets`` (n_keys + 1 uint32) and ``entries`` (PPF_ENTRY) on the device."""
        if self.offsets is None:
            n = len(self.points)
            pts = self.device_points()
            offsets = DeviceVector(self.params.n_keys + 1, np.uint32)
            entries = DeviceVector(max(1, n * (n - 1)), PPF_ENTRY)
            ne = C.c_uint32(0)
            check(_lib.load().pr_ppf_model_build_dev(C.addressof(self.params), pts.data(), self._normals_dev.data(), n, offsets.data(), entries.data(), C.byref(ne)))
            self.offsets, self.entries, self.n_entries = offsets, entries, ne.value
        return self

    def table(self):
        """(offsets uint32[n_keys + 1], entries PPF_ENTRY[n_entries]) read back from the device (tests and tools)."""
        self.build()
        return self.offsets.to_host(), self.entries.to_host()[:self.n_entries]


def ppf_scene_points(scene: "Scene_projective", stride: int):
    """``pr_ppf_scene_points_dev``: (points, normals, n) -- two DeviceVectors with room for ``PPF_MAX_SCENE_POINTS`` points (3 float32 each), the
    first ``n`` filled: every ``stride``-th column and row of a full-frame projective scene with a normal and a depth, in mm, row-major."""
    if scene.kind != SCENE_PROJ:
        raise ValueError("ppf_scene_points takes a full-frame Scene_projective")
    pts = DeviceVector(PPF_MAX_SCENE_POINTS * 3, np.float32)
    nrm = DeviceVector(PPF_MAX_SCENE_POINTS * 3, np.float32)
    d = scene.desc()
    n = C.c_uint32(0)
    check(_lib.load().pr_ppf_scene_points_dev(C.addressof(d), int(stride), pts.data(), nrm.data(), C.byref(n)))
    return pts, nrm, n.value


def ppf_cloud_points(scene: "Scene_nn", stride: int):
    """``pr_ppf_cloud_points_dev``: ``ppf_scene_points`` for a kd-tree scene (one made from a point cloud above all) -- (points, normals, n): the
    points 0, ``stride``, 2 ``stride``, ... of tree order that have a normal, in index order, in mm."""
    if scene.kind != SCENE_NN:
        raise ValueError("ppf_cloud_points takes a Scene_nn")
    pts = DeviceVector(PPF_MAX_SCENE_POINTS * 3, np.float32)
    nrm = DeviceVector(PPF_MAX_SCENE_POINTS * 3, np.float32)
    d = scene.desc()
    n = C.c_uint32(0)
    check(_lib.load().pr_ppf_cloud_points_dev(C.addressof(d), int(stride), pts.data(), nrm.data(), C.byref(n)))
    return pts, nrm, n.value


def ppf_vote(ppf_model: PPFModel, scene_points: DeviceVector, scene_normals: DeviceVector, n_scene: int, ref_first: int = 0, ref_stride: int = 1,
             n_refs: Optional[int] = None, n_peaks: int = 1, want_acc: bool = False):
    """``pr_ppf_vote``: (peaks PPF_PEAK[n_refs, n_peaks], poses float32[n_refs, n_peaks, 4, 4]) of the references ``ref_first + j * ref_stride``
    (``n_refs=None``: as many as fit); with ``want_acc`` also the accumulators, uint32[n_refs, n_model, n_alpha] (tests and tools)."""
    ppf_model.build()
    if n_refs is None:
        n_refs = 0 if ref_first >= n_scene or ref_stride < 1 else (n_scene - 1 - ref_first) // ref_stride + 1
    n_model, n_alpha = len(ppf_model.points), ppf_model.params.n_alpha
    peaks = np.zeros((n_refs, n_peaks), PPF_PEAK)
    poses = np.zeros((n_refs, n_peaks, 4, 4), np.float32)
    acc = DeviceVector(max(1, n_refs * n_model * n_alpha), np.uint32) if want_acc else None
    check(_lib.load().pr_ppf_vote(C.addressof(ppf_model.params), ppf_model.offsets.data(), ppf_model.entries.data(), ptr(ppf_model.points), ptr(ppf_model.normals),
                                  n_model, scene_points.data(), scene_normals.data(), int(n_scene), int(ref_first), int(ref_stride), int(n_refs), int(n_peaks),
                                  ptr(peaks), ptr(poses), acc.data() if want_acc else None))
    if want_acc:
        return peaks, poses, acc.to_host()[:n_refs * n_model * n_alpha].reshape(n_refs, n_model, n_alpha)
    return peaks, poses


def generate_hypotheses(ppf_model: PPFModel, scene: "Scene_projective", stride: int = 4, ref_stride: int = 5, n_peaks: int = 1, max_hypotheses: int = 256,
                        merge_mm: Optional[float] = None, scene_sample=None):
    """Pose hypotheses from a frame and a mesh alone: sample the scene (``stride``), vote with every ``ref_stride``-th sample as a reference, order
    the peaks by votes (descending, then by index), merge duplicates with ``pose_distance_matrix`` + ``merge_duplicates`` over the model's sample
    points (``merge_mm`` defaults to ``dist_step_mm``), add the votes of each merged group onto its representative and order again.  Returns
    (poses float32[n, 4, 4], votes int64[n]), n <= ``max_hypotheses``: ready for ``refine_batch`` and ``score_poses``.  The vote sum is only the
    order in which hypotheses are handed on; ``rank_hypotheses`` stays the one definition of better after scoring.  ``scene_sample``: a
    ``(points, normals, n)`` triple as ``ppf_scene_points`` / ``ppf_cloud_points`` return it, taken in place of sampling ``scene`` (which may then
    be None, and ``stride`` is not read)."""
    pts, nrm, n_scene = ppf_scene_points(scene, stride) if scene_sample is None else scene_sample
    if n_scene == 0:
        return np.zeros((0, 4, 4), np.float32), np.zeros(0, np.int64)
    n_refs = (n_scene - 1) // ref_stride + 1
    if n_refs * n_peaks > POSE_DIST_MAX_POSES:
        raise ValueError(f"{n_refs} references x {n_peaks} peaks exceed POSE_DIST_MAX_POSES = {POSE_DIST_MAX_POSES}: raise stride or ref_stride")
    peaks, poses = ppf_vote(ppf_model, pts, nrm, n_scene, 0, ref_stride, n_refs, n_peaks)
    return _merged_hypotheses(ppf_model, peaks, poses, max_hypotheses, merge_mm)


def _merged_hypotheses(ppf_model: PPFModel, peaks, poses, max_hypotheses: int, merge_mm: Optional[float]):
    """The tail of ``generate_hypotheses`` and, per model, of ``generate_hypotheses_multi``: one model's peaks and poses (any leading shape) to its
    list -- the peaks with votes in the order (votes descending, index ascending), duplicates merged over the model's own sample points, the
    votes of a group summed onto its representative, ordered again, cut to ``max_hypotheses``."""
    votes = peaks["votes"].reshape(-1).astype(np.int64)
    poses = poses.reshape(-1, 4, 4)
    live = np.flatnonzero(votes > 0)
    if len(live) == 0:
        return np.zeros((0, 4, 4), np.float32), np.zeros(0, np.int64)
    votes, poses = votes[live], np.ascontiguousarray(poses[live])
    order = np.argsort(-votes, kind="stable")
    dist = pose_distance_matrix(ppf_model.device_points(), poses)
    kept, rep = merge_duplicates(order, dist, ppf_model.dist_step_mm if merge_mm is None else merge_mm)
    total = np.zeros(len(votes), np.int64)
    np.add.at(total, rep, votes)
    kept = kept[np.argsort(-total[kept], kind="stable")][:max_hypotheses]
    return poses[kept], total[kept]


def ppf_vote_multi(ppf_models, scene_points: DeviceVector, scene_normals: DeviceVector, n_scene: int, ref_first: int = 0, ref_stride: int = 1,
                   n_refs: Optional[int] = None, n_peaks: int = 1, want_acc: bool = False):
    """``pr_ppf_vote_multi``: a list of ``PPFModel`` over one scene sample in one call -- (peaks PPF_PEAK[n_models, n_refs, n_peaks], poses
    float32[n_models, n_refs, n_peaks, 4, 4]), slice k byte for byte what ``ppf_vote(ppf_models[k], ...)`` returns; with ``want_acc`` also a list of
    the models' accumulators, uint32[n_refs, n_model_k, n_alpha_k] (tests and tools).  Every model's table is built on first use."""
    models = list(ppf_models)
    if len(models) > PPF_MAX_MODELS:
        raise ValueError(f"ppf_vote_multi: {len(models)} models, at most PPF_MAX_MODELS = {PPF_MAX_MODELS}")
    for m in models:
        m.build()
    if n_refs is None:
        n_refs = 0 if ref_first >= n_scene or ref_stride < 1 else (n_scene - 1 - ref_first) // ref_stride + 1
    table = (PPFModelDesc * max(1, len(models)))()
    for k, m in enumerate(models):                                  # (the models themselves keep the host arrays and the device tables alive)
        table[k] = PPFModelDesc(C.addressof(m.params), m.offsets.data(), m.entries.data(), ptr(m.points), ptr(m.normals), len(m.points), 0)
    peaks = np.zeros((len(models), n_refs, n_peaks), PPF_PEAK)
    poses = np.zeros((len(models), n_refs, n_peaks, 4, 4), np.float32)
    cells = [len(m.points) * m.params.n_alpha for m in models]
    acc = DeviceVector(max(1, n_refs * sum(cells)), np.uint32) if want_acc else None
    check(_lib.load().pr_ppf_vote_multi(C.addressof(table), len(models), scene_points.data(), scene_normals.data(), int(n_scene), int(ref_first), int(ref_stride),
                                        int(n_refs), int(n_peaks), ptr(peaks), ptr(poses), acc.data() if want_acc else None))
    if not want_acc:
        return peaks, poses
    flat, at, accs = acc.to_host(), 0, []
    for m, c in zip(models, cells):
        accs.append(flat[at:at + n_refs * c].reshape(n_refs, len(m.points), m.params.n_alpha))
        at += n_refs * c
    return peaks, poses, accs


def generate_hypotheses_multi(ppf_models, scene: "Scene_projective", stride: int = 4, ref_stride: int = 5, n_peaks: int = 1, max_hypotheses: int = 256,
                              merge_mm: Optional[float] = None, scene_sample=None):
    """``generate_hypotheses`` for several meshes in one frame: one scene sample, ONE vote call (``ppf_vote_multi``), then per model exactly
    ``generate_hypotheses``' ordering, merge (over that model's own sample points, at its ``dist_step_mm`` unless ``merge_mm`` is given) and vote
    summing.  Returns (mesh_index int32[n], poses float32[n, 4, 4], votes int64[n]) grouped by model in table order, votes descending within a
    model, at most ``max_hypotheses`` per model: the slice of model k equals ``generate_hypotheses(ppf_models[k], scene, ...)`` byte for byte, and
    (mesh_index, poses) go straight to ``refine_batch_multi`` / ``score_poses_multi`` with the models' meshes in the same order.
    ``scene_sample``: as in ``generate_hypotheses``."""
    models = list(ppf_models)
    if len(models) == 0:
        raise ValueError("generate_hypotheses_multi: no models")
    empty = (np.zeros(0, np.int32), np.zeros((0, 4, 4), np.float32), np.zeros(0, np.int64))
    pts, nrm, n_scene = ppf_scene_points(scene, stride) if scene_sample is None else scene_sample
    if n_scene == 0:
        return empty
    n_refs = (n_scene - 1) // ref_stride + 1
    if n_refs * n_peaks > POSE_DIST_MAX_POSES:                      # per model: every model's merge is a pose_distance_matrix of its own
        raise ValueError(f"{n_refs} references x {n_peaks} peaks exceed POSE_DIST_MAX_POSES = {POSE_DIST_MAX_POSES}: raise stride or ref_stride")
    peaks, poses = ppf_vote_multi(models, pts, nrm, n_scene, 0, ref_stride, n_refs, n_peaks)
    lists = [_merged_hypotheses(m, peaks[k], poses[k], max_hypotheses, merge_mm) for k, m in enumerate(models)]
    return (np.concatenate([np.full(len(v), k, np.int32) for k, (_, v) in enumerate(lists)]), np.concatenate([p for p, _ in lists]),
            np.concatenate([v for _, v in lists]))


# What the frame stages' wrappers (clouds, planes, segments, depth conditioning, reprojection) share.
def _params(params, kw, factory):
    """A stage's checked parameter block: the caller's, or ``factory`` (``CloudParams``, ``PlaneParams``, ...) over the keywords."""
    if params is not None and kw:
        raise ValueError("pass either a parameter block or keyword parameters, not both")
    return params if params is not None else factory(**kw)


def _host_depth(depth, n_px: int) -> np.ndarray:
    dep = np.ascontiguousarray(depth)
    if dep.dtype not in (np.uint16, np.int32):
        raise ValueError("scene depth must be CV_16U or CV_32S")
    if dep.size != n_px:
        raise ValueError(f"depth holds {dep.size} values, expected {n_px}")
    return dep


def _depth_out(depth_out: Optional[DeviceVector], n_px: int, dtype) -> DeviceVector:
    """Where a stage's depth goes: the caller's ``depth_out``, checked, or a new DeviceVector."""
    out = depth_out if depth_out is not None else DeviceVector(n_px, dtype)
    if out.dtype != dtype or out.size() != n_px:
        raise ValueError(f"depth_out must have the depth's dtype and size ({np.dtype(dtype)}, {n_px} values)")
    return out


def _with_extras(base, extras, tail=()) -> tuple:
    """A stage's result tuple, device or host form: ``base``, the value of every wanted ``(want, value)`` pair of ``extras``, ``tail``."""
    return tuple(base) + tuple(v for want, v in extras if want) + tuple(tail)


# ------------------------------------------------------------------------------------------------
# scenes from point clouds: exact k nearest neighbours over the scene's kd-tree and a PCA normal per point (pr_cloud_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def CloudParams(k: int = 16, max_radius: float = float("inf"), min_neighbours: int = 3, line_ratio: float = 1e-4, viewpoint=(0.0, 0.0, 0.0)) -> CloudParamsDesc:
    """``pr_cloud_describe``: the checked parameter block of ``cloud_knn`` / ``cloud_normals`` and their host twins."""
    out = CloudParamsDesc()
    vp = _f32(viewpoint, -1)
    if vp.size != 3:
        raise ValueError("viewpoint: three coordinates")
    check(_lib.load().pr_cloud_describe(int(k), float(max_radius), int(min_neighbours), float(line_ratio), ptr(vp), C.addressof(out)))
    return out


def _cloud_counts(c: CloudCounts) -> dict:
    return {"points": int(c.points), "with_normal": int(c.with_normal), "too_few": int(c.too_few), "degenerate": int(c.degenerate)}


def cloud_knn(scene: "Scene_nn", params: Optional[CloudParamsDesc] = None, **kw):
    """``pr_cloud_knn_dev``: the exact ``k`` nearest neighbours of every point of a kd-tree scene among the scene's own points (itself included),
    within ``max_radius`` -- (idx uint32[n, k], d2 float32[n, k], count uint32[n]) read back from the device; unused slots hold ``KNN_NONE`` / 0."""
    if scene.kind != SCENE_NN:
        raise ValueError("cloud_knn takes a Scene_nn")
    p = _params(params, kw, CloudParams)
    d = scene.desc()
    n, k = int(d.n_points), int(p.k)
    idx, d2, cnt = DeviceVector(n * k, np.uint32), DeviceVector(n * k, np.float32), DeviceVector(n, np.uint32)
    check(_lib.load().pr_cloud_knn_dev(C.addressof(d), C.addressof(p), idx.data(), d2.data(), cnt.data()))
    return idx.to_host().reshape(n, k), d2.to_host().reshape(n, k), cnt.to_host()


def cloud_normals(scene: "Scene_nn", params: Optional[CloudParamsDesc] = None, normal_out: Optional[DeviceVector] = None, want_variation: bool = False,
                  in_place: bool = False, **kw):
    """``pr_cloud_normals_dev``: the PCA normal of every point of a kd-tree scene from its k nearest neighbours -- (normals, variation, counts):
    a ``DeviceVector`` of 3 n floats (``normal_out`` if given; the scene's own normal array with ``in_place``), the surface variation as a
    ``DeviceVector`` of n floats or None, and the four counts as a dict."""
    if scene.kind != SCENE_NN:
        raise ValueError("cloud_normals takes a Scene_nn")
    p = _params(params, kw, CloudParams)
    d = scene.desc()
    n = int(d.n_points)
    out = scene.normal_buffer if in_place else (normal_out if normal_out is not None else DeviceVector(n * 3, np.float32))
    if out.size() < n * 3:
        raise ValueError(f"normal_out holds {out.size()} floats, the scene needs {n * 3}")
    var = DeviceVector(n, np.float32) if want_variation else None
    counts = CloudCounts()
    check(_lib.load().pr_cloud_normals_dev(C.addressof(d), C.addressof(p), out.data(), var.data() if var is not None else None, C.addressof(counts)))
    return out, var, _cloud_counts(counts)


def kdtree_build_host(points, max_leaf: int = 10):
    """``pr_kdtree_build`` on host points: (points float32[n, 3] in tree order, nodes KDNODE[n_nodes]) -- what the host twins below take, and
    byte for byte what ``pr_kdtree_build_dev`` makes of the same points."""
    pts = np.array(points, np.float32, order="C").reshape(-1, 3)
    nrm = np.zeros_like(pts)
    nodes = np.zeros(2 * len(pts) + 1, KDNODE)
    nn = C.c_uint32()
    check(_lib.load().pr_kdtree_build(ptr(pts), ptr(nrm), len(pts), int(max_leaf), ptr(nodes), len(nodes), C.byref(nn)))
    return pts, np.ascontiguousarray(nodes[:nn.value])


def cloud_knn_host(points, nodes, params: Optional[CloudParamsDesc] = None, **kw):
    """``pr_cloud_knn_host``: ``cloud_knn`` on the CPU over host points in tree order and their ``KDNODE`` array (``kdtree_build_host``)."""
    p = _params(params, kw, CloudParams)
    pts, nd = _f32(points).reshape(-1, 3), np.ascontiguousarray(nodes, KDNODE)
    n, k = len(pts), int(p.k)
    idx, d2, cnt = np.zeros((n, k), np.uint32), np.zeros((n, k), np.float32), np.zeros(n, np.uint32)
    check(_lib.load().pr_cloud_knn_host(ptr(pts), n, ptr(nd), len(nd), C.addressof(p), ptr(idx), ptr(d2), ptr(cnt)))
    return idx, d2, cnt


def cloud_normals_host(points, nodes, params: Optional[CloudParamsDesc] = None, **kw):
    """``pr_cloud_normals_host``: (normals float32[n, 3], variation float32[n], counts dict) on the CPU, byte for byte ``cloud_normals``."""
    p = _params(params, kw, CloudParams)
    pts, nd = _f32(points).reshape(-1, 3), np.ascontiguousarray(nodes, KDNODE)
    nrm, var, counts = np.zeros((len(pts), 3), np.float32), np.zeros(len(pts), np.float32), CloudCounts()
    check(_lib.load().pr_cloud_normals_host(ptr(pts), len(pts), ptr(nd), len(nd), C.addressof(p), ptr(nrm), ptr(var), C.addressof(counts)))
    return nrm, var, _cloud_counts(counts)


# ------------------------------------------------------------------------------------------------
# support planes: the dominant planes of a frame, their labels and the cleared depth (pr_plane_* / pr_scene_planes_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def PlaneParams(stride: int = 4, cand_stride: int = 16, tau_mm: float = 3.0, label_tau_mm: float = 6.0, cos_min: float = 0.9, min_support: int = 500,
                n_planes: int = 1, drop_behind: bool = True) -> PlaneParamsDesc:
    """``pr_plane_describe`` (host only): the parameters of a peel, checked.  The defaults are for a 640 x 480 frame in mm with a table or a wall:
    every 4th pixel a sample, every 16th sample a candidate, 3 mm to support a candidate and 6 mm to take a fitted plane's label, normals within
    about 26 degrees (``cos_min=-2`` switches the normal test off), at least 500 supporting samples, and what lies behind plane 1 dropped."""
    pp = PlaneParamsDesc()
    check(_lib.load().pr_plane_describe(int(stride), int(cand_stride), float(tau_mm), float(label_tau_mm), float(cos_min), int(min_support), int(n_planes),
                                        int(bool(drop_behind)), C.addressof(pp)))
    return pp


def plane_from_moments(moments):
    """``pr_plane_from_moments`` (host only): (normal float64[3], offset_mm, rms_mm, eig float64[3]) of the ten int64 moments n, Sx, Sy, Sz, Sxx, Sxy,
    Sxz, Syy, Syz, Szz on the 1/16 mm grid.  ``eig[0]`` is the plane's eigenvalue (the smallest), the other two follow in index order."""
    m = np.ascontiguousarray(moments, dtype=np.int64).reshape(10)
    nrm, eig = np.zeros(3, np.float64), np.zeros(3, np.float64)
    off, rms = C.c_double(0.0), C.c_double(0.0)
    check(_lib.load().pr_plane_from_moments(ptr(m), ptr(nrm), C.byref(off), C.byref(rms), ptr(eig)))
    return nrm, off.value, rms.value, eig


def scene_planes(scene: "Scene_projective", scene_depth, params: Optional[PlaneParamsDesc] = None, depth_out: Optional[DeviceVector] = None,
                 want_moments: bool = False, want_supports: bool = False, **kw):
    """``pr_scene_planes_dev``: the dominant planes of a full-frame projective scene and its depth frame (a DeviceVector or a host image, uint16 or
    int32).  Returns (planes PLANE[n_found], labels DeviceVector uint8[width * height], cleared DeviceVector of the depth's dtype): ``labels`` holds
    the round (1-based) that took a pixel, ``PLANE_BEHIND``, ``PLANE_NO_DEPTH`` or 0; ``cleared`` is the depth with every labelled pixel set to 0 --
    it goes as it is into ``init_Scene_projective_device``, ``init_Scene_nn_device`` and the scorers.  ``depth_out``: where the cleared depth goes
    (the input itself is allowed).  ``want_moments`` adds int64[n_found, 10], ``want_supports`` the support table uint32[n_planes, PLANE_MAX_CANDIDATES]
    (tests and tools; a row's first n_candidates words are used).  Parameters: a ``PlaneParams`` or its keywords."""
    if scene.kind != SCENE_PROJ:
        raise ValueError("scene_planes takes a full-frame Scene_projective")
    pp = _params(params, kw, PlaneParams)
    W, H = scene.width, scene.height
    sd = _scene_depth_dev(scene_depth, W, H)
    out = _depth_out(depth_out, W * H, sd.dtype)
    labels = DeviceVector(W * H, np.uint8)
    planes = np.zeros(PLANE_MAX_PLANES, PLANE)
    moments = np.zeros((PLANE_MAX_PLANES, 10), np.int64)
    sup = DeviceVector(pp.n_planes * PLANE_MAX_CANDIDATES, np.uint32) if want_supports else None
    d = scene.desc()
    n = C.c_uint32(0)
    check(_lib.load().pr_scene_planes_dev(C.addressof(d), sd.data(), int(sd.dtype == np.int32), C.addressof(pp), labels.data(), out.data(), ptr(planes),
                                          ptr(moments), sup.data() if want_supports else None, C.byref(n)))
    return _with_extras((planes[:n.value].copy(), labels, out),
                        ((want_moments, moments[:n.value].copy()), (want_supports, sup.to_host().reshape(pp.n_planes, PLANE_MAX_CANDIDATES) if want_supports else None)))


def scene_planes_host(pcd, normal, scene_depth, width: int, height: int, params: Optional[PlaneParamsDesc] = None, want_moments: bool = False,
                      want_supports: bool = False, **kw):
    """``pr_scene_planes_host``: ``scene_planes`` over host arrays (pcd and normal float32[height * width, 3] as ``init_Scene_projective_cuda`` keeps
    them in ``pcd_host`` / ``normal_host``, the depth image uint16 or int32), on the CPU, from the same definition.  Returns (planes, labels
    uint8[height, width], cleared depth[height, width]) and on request moments and the support table uint32[n_planes, PLANE_MAX_CANDIDATES]; runs without a GPU."""
    pp = _params(params, kw, PlaneParams)
    p, m = _f32(pcd, (-1, 3)), _f32(normal, (-1, 3))
    dep = _host_depth(scene_depth, width * height)
    if len(p) != width * height or len(m) != width * height:
        raise ValueError(f"pcd and normal must hold {width} x {height} pixels")
    labels = np.zeros((height, width), np.uint8)
    cleared = np.zeros((height, width), dep.dtype)
    planes = np.zeros(PLANE_MAX_PLANES, PLANE)
    moments = np.zeros((PLANE_MAX_PLANES, 10), np.int64)
    sup = np.zeros((pp.n_planes, PLANE_MAX_CANDIDATES), np.uint32)
    n = C.c_uint32(0)
    check(_lib.load().pr_scene_planes_host(ptr(p), ptr(m), ptr(dep), int(dep.dtype == np.int32), width, height, C.addressof(pp), ptr(labels), ptr(cleared),
                                           ptr(planes), ptr(moments), ptr(sup) if want_supports else None, C.byref(n)))
    return _with_extras((planes[:n.value].copy(), labels, cleared), ((want_moments, moments[:n.value].copy()), (want_supports, sup)))


# ------------------------------------------------------------------------------------------------
# scene segments: the depth-connected components of a frame, their labels, boxes and the depth of chosen ones (pr_segment_* / pr_scene_segments_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def SegmentParams(jump_mm: int = 10, min_pixels: int = 256, max_segments: int = 64) -> SegmentParamsDesc:
    """``pr_segment_describe`` (host only): the parameters of a labelling, checked.  The defaults are for a 640 x 480 frame in mm whose support planes
    are cleared: 4-neighbours within 10 mm of depth belong together, a blob of fewer than 256 pixels is dropped, the 64 largest blobs get a label."""
    sp = SegmentParamsDesc()
    check(_lib.load().pr_segment_describe(int(jump_mm), int(min_pixels), int(max_segments), C.addressof(sp)))
    return sp


def scene_segments(scene_depth, width: int, height: int, params: Optional[SegmentParamsDesc] = None, want_roots: bool = False, **kw):
    """``pr_scene_segments_dev``: the depth-connected components of a depth frame (a DeviceVector or a host image, uint16 or int32; typically
    ``scene_planes``' cleared depth).  Returns (segments SEGMENT[n_found], labels DeviceVector uint16[width * height], counts): ``labels`` holds 0
    where nothing is measured, k for the k-th largest component and ``SEGMENT_DROPPED`` for the rest; ``counts`` is (n_found, n_qualifying,
    n_components).  ``want_roots`` adds, before the counts, a DeviceVector uint32[width * height] with every pixel's root (tests and tools).
    Parameters: a ``SegmentParams`` or its keywords."""
    sp = _params(params, kw, SegmentParams)
    sd = _scene_depth_dev(scene_depth, width, height)
    labels = DeviceVector(width * height, np.uint16)
    roots = DeviceVector(width * height, np.uint32) if want_roots else None
    segs = np.zeros(sp.max_segments, SEGMENT)
    n, nq, nc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().pr_scene_segments_dev(sd.data(), int(sd.dtype == np.int32), width, height, C.addressof(sp), labels.data(), roots.data() if want_roots else None,
                                            ptr(segs), C.byref(n), C.byref(nq), C.byref(nc)))
    return _with_extras((segs[:n.value].copy(), labels), ((want_roots, roots),), ((n.value, nq.value, nc.value),))


def scene_segments_host(depth, width: int, height: int, params: Optional[SegmentParamsDesc] = None, want_roots: bool = False, **kw):
    """``pr_scene_segments_host``: ``scene_segments`` over a host image (uint16 or int32), on the CPU, from the same definition.  Returns (segments,
    labels uint16[height, width][, roots uint32[height, width]], counts); runs without a GPU."""
    sp = _params(params, kw, SegmentParams)
    dep = _host_depth(depth, width * height)
    labels = np.zeros((height, width), np.uint16)
    roots = np.zeros((height, width), np.uint32) if want_roots else None
    segs = np.zeros(sp.max_segments, SEGMENT)
    n, nq, nc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().pr_scene_segments_host(ptr(dep), int(dep.dtype == np.int32), width, height, C.addressof(sp), ptr(labels), ptr(roots) if want_roots else None,
                                             ptr(segs), C.byref(n), C.byref(nq), C.byref(nc)))
    return _with_extras((segs[:n.value].copy(), labels), ((want_roots, roots),), ((n.value, nq.value, nc.value),))


def segment_depth(labels: DeviceVector, scene_depth, keep, depth_out: Optional[DeviceVector] = None) -> DeviceVector:
    """``pr_segment_depth_dev``: the depth frame with everything but the segments ``keep`` (a label or a list of labels, 1-based) set to 0; it goes as it
    is into ``init_Scene_projective_device``, ``init_Scene_nn_device``, the PPF sampler and the scorers.  ``depth_out``: where it goes (the input
    itself is allowed); default a new DeviceVector of the depth's dtype."""
    n_px = labels.size()
    sd = _scene_depth_dev(scene_depth, n_px, 1)
    if labels.dtype != np.uint16:
        raise ValueError("labels must be uint16")
    out = _depth_out(depth_out, n_px, sd.dtype)
    ks = [int(k) for k in np.atleast_1d(np.asarray(keep)).reshape(-1)]
    if any(k < 1 or k > SEGMENT_MAX for k in ks):
        raise ValueError(f"a kept label must be 1 .. SEGMENT_MAX = {SEGMENT_MAX}")
    table = np.zeros((max(ks) if ks else 0) + 1, np.uint8)
    table[ks] = 1
    check(_lib.load().pr_segment_depth_dev(labels.data(), sd.data(), int(sd.dtype == np.int32), n_px, ptr(table), len(table), out.data()))
    return out


def segment_roi(segment, width: int, height: int, margin: int = 0):
    """``pr_segment_roi`` (host only): a SEGMENT record's pixel box grown by ``margin`` and clipped to the frame, as the (x, y, width, height) tuple
    every ``roi`` argument takes."""
    rec = np.zeros(1, SEGMENT)
    rec[0] = segment
    r = Roi()
    check(_lib.load().pr_segment_roi(ptr(rec), width, height, int(margin), C.byref(r)))
    return (r.x, r.y, r.width, r.height)


# ------------------------------------------------------------------------------------------------
# depth conditioning: fuse frames of one view, drop flying pixels, median, fill holes (pr_depth_fuse_* / pr_depth_filter_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def DepthFilterParams(min_mm: int = 0, max_mm: int = 0, tol_mm: int = 0, tol_permille: int = 0, fly_min_support: int = 0, radius: int = 0,
                      fill_min: int = 0) -> DepthFilterParamsDesc:
    """``pr_depth_filter_describe`` (host only): the parameters of a filter call, checked.  Every stage is off by default: no gate (``min_mm`` 0,
    ``max_mm`` 0 = no upper gate), no flying-pixel test (``fly_min_support`` 0), no median and no fill (``radius`` 0, ``fill_min`` 0).
    ``tol(d) = tol_mm + d * tol_permille // 1000`` is the depth difference within which two pixels count as one surface."""
    dp = DepthFilterParamsDesc()
    check(_lib.load().pr_depth_filter_describe(int(min_mm), int(max_mm), int(tol_mm), int(tol_permille), int(fly_min_support), int(radius), int(fill_min),
                                               C.addressof(dp)))
    return dp


def depth_filter(depth, width: int, height: int, params: Optional[DepthFilterParamsDesc] = None, depth_out: Optional[DeviceVector] = None,
                 want_flags: bool = False, **kw):
    """``pr_depth_filter_dev``: a depth frame (a DeviceVector or a host image, uint16 or int32) with its range gate applied, its flying pixels
    removed, an edge-preserving median over what is left and its holes filled.  Returns (cleaned DeviceVector of the depth's dtype[, flags
    DeviceVector uint8[width * height]], counts): ``flags`` (``want_flags``) holds every pixel's ``DEPTH_*`` code, ``counts`` is a tuple of the six
    codes' pixel counts.  The cleaned frame goes as it is into ``init_Scene_projective_device``, ``init_Scene_nn_device``, ``scene_planes``,
    ``scene_segments``, ``generate_hypotheses`` and the scorers.  ``depth_out``: where it goes (never the input: the filter is a stencil); default
    a new DeviceVector.  Parameters: a ``DepthFilterParams`` or its keywords."""
    dp = _params(params, kw, DepthFilterParams)
    sd = _scene_depth_dev(depth, width, height)
    out = _depth_out(depth_out, width * height, sd.dtype)
    flags = DeviceVector(width * height, np.uint8) if want_flags else None
    cnt = DepthFilterCounts()
    check(_lib.load().pr_depth_filter_dev(sd.data(), int(sd.dtype == np.int32), width, height, C.addressof(dp), out.data(), flags.data() if want_flags else None,
                                          C.addressof(cnt)))
    return _with_extras((out,), ((want_flags, flags),), (tuple(cnt.n),))


def depth_filter_host(depth, width: int, height: int, params: Optional[DepthFilterParamsDesc] = None, want_flags: bool = False, **kw):
    """``pr_depth_filter_host``: ``depth_filter`` over a host image (uint16 or int32), on the CPU, from the same definition.  Returns (cleaned
    depth[height, width][, flags uint8[height, width]], counts); runs without a GPU."""
    dp = _params(params, kw, DepthFilterParams)
    dep = _host_depth(depth, width * height)
    out = np.zeros((height, width), dep.dtype)
    flags = np.zeros((height, width), np.uint8) if want_flags else None
    cnt = DepthFilterCounts()
    check(_lib.load().pr_depth_filter_host(ptr(dep), int(dep.dtype == np.int32), width, height, C.addressof(dp), ptr(out), ptr(flags) if want_flags else None,
                                           C.addressof(cnt)))
    return _with_extras((out,), ((want_flags, flags),), (tuple(cnt.n),))


def depth_fuse(frames, width: int, height: int, min_frames: int = 1, depth_out: Optional[DeviceVector] = None, want_count: bool = False):
    """``pr_depth_fuse_dev``: the per-pixel lower median over 1 .. ``DEPTH_FUSE_MAX`` depth frames of ONE view (DeviceVectors or host images of one
    dtype, uint16 or int32), taken over the frames that measured the pixel; 0 where fewer than ``min_frames`` did.  Returns the fused DeviceVector,
    with ``want_count`` (fused, count DeviceVector uint8[width * height]).  ``depth_out``: where it goes (one of the frames is allowed)."""
    fs = [_scene_depth_dev(f, width, height) for f in frames]
    if not fs or any(f.dtype != fs[0].dtype for f in fs):
        raise ValueError("depth_fuse takes at least one frame, all of one dtype")
    n_px = width * height
    out = _depth_out(depth_out, n_px, fs[0].dtype)
    count = DeviceVector(n_px, np.uint8) if want_count else None
    table = (C.c_void_p * len(fs))(*[f.data() for f in fs])
    check(_lib.load().pr_depth_fuse_dev(C.addressof(table), len(fs), int(fs[0].dtype == np.int32), n_px, int(min_frames), out.data(),
                                        count.data() if want_count else None))
    return (out, count) if want_count else out


def depth_fuse_host(frames, width: int, height: int, min_frames: int = 1, want_count: bool = False):
    """``pr_depth_fuse_host``: ``depth_fuse`` over host images, on the CPU, from the same definition.  Returns the fused depth[height, width], with
    ``want_count`` (fused, count uint8[height, width]); runs without a GPU."""
    n_px = width * height
    fs = [_host_depth(f, n_px) for f in frames]
    if not fs or any(f.dtype != fs[0].dtype for f in fs):
        raise ValueError("depth_fuse_host takes at least one frame, all of one dtype")
    out = np.zeros((height, width), fs[0].dtype)
    count = np.zeros((height, width), np.uint8) if want_count else None
    table = (C.c_void_p * len(fs))(*[ptr(f) for f in fs])
    check(_lib.load().pr_depth_fuse_host(C.addressof(table), len(fs), int(fs[0].dtype == np.int32), n_px, int(min_frames), ptr(out), ptr(count) if want_count else None))
    return (out, count) if want_count else out


# ------------------------------------------------------------------------------------------------
# reprojection: depth frames of other cameras and bare clouds into the depth frame of one camera (pr_depth_reproject_*; the definition is in include/pose_refine.h)
# ------------------------------------------------------------------------------------------------
def ReprojectParams(splat: int = 1, min_mm: int = 0, max_mm: int = 0, tol_mm: int = 0, tol_permille: int = 0, occl_radius: int = 0,
                    occl_min_front: int = 0) -> ReprojectParamsDesc:
    """``pr_reproject_describe`` (host only): the parameters of a reprojection, checked.  ``splat`` 1 .. 3 is the side of the square of pixels a
    sample writes; ``min_mm`` / ``max_mm`` gate the reprojected depth (``max_mm`` 0: no gate but the depth type's); the visibility stage is off by
    default (``occl_min_front`` 0): with ``occl_radius`` 1 .. 2 a pixel is hidden when ``occl_min_front`` pixels of its window are nearer by more
    than ``tol(d) = tol_mm + d * tol_permille // 1000``."""
    rp = ReprojectParamsDesc()
    check(_lib.load().pr_reproject_describe(int(splat), int(min_mm), int(max_mm), int(tol_mm), int(tol_permille), int(occl_radius), int(occl_min_front),
                                            C.addressof(rp)))
    return rp


def _pinhole(K):
    k = _f32(K, -1)
    if k.size != 9:
        raise ValueError("K must be a 3 x 3 intrinsic matrix")
    return float(k[0]), float(k[4]), float(k[2]), float(k[5])


class ReprojectSource:
    """One source of ``depth_reproject``: ``ReprojectSource.frame`` or ``ReprojectSource.cloud``.  ``T`` is the 4 x 4 transform from the source's
    camera to the target's, translation in metres; default the identity."""

    def __init__(self, kind: int, data, T=None, width: int = 0, height: int = 0, K=None, n_points: int = 0, offset_bytes: int = 0):
        self.kind, self.data, self.width, self.height, self.n_points, self.offset_bytes = kind, data, int(width), int(height), int(n_points), int(offset_bytes)
        self.pinhole = _pinhole(K) if K is not None else (0.0, 0.0, 0.0, 0.0)
        self.T = _f32(np.eye(4) if T is None else T, -1)
        if self.T.size != 16:
            raise ValueError("T must be a 4 x 4 matrix")

    @classmethod
    def frame(cls, depth, width: int, height: int, K, T=None, offset_elems: int = 0) -> "ReprojectSource":
        """A depth frame (a DeviceVector or a host image, uint16 or int32) of ``width`` x ``height`` pixels with intrinsics ``K``; ``offset_elems``
        selects an image of a stack, as in ``depth2cloud``."""
        dt = depth.dtype
        if dt not in (np.uint16, np.int32):
            raise ValueError("a frame source must be CV_16U or CV_32S")
        n = depth.size() if isinstance(depth, DeviceVector) else depth.size
        if offset_elems < 0 or n - offset_elems < width * height or (offset_elems == 0 and n != width * height):
            raise ValueError(f"a buffer of {n} values holds no {width} x {height} frame at element {offset_elems}")
        return cls(SRC_DEPTH_I32 if dt == np.int32 else SRC_DEPTH_U16, depth, T, width, height, K, offset_bytes=offset_elems * dt.itemsize)

    @classmethod
    def cloud(cls, points, T=None, offset_points: int = 0) -> "ReprojectSource":
        """A bare cloud: an (n, 3) float32 host array or a DeviceVector of 3 n floats, in metres, from point ``offset_points`` on."""
        if isinstance(points, DeviceVector):
            if points.dtype != np.float32 or points.size() % 3:
                raise ValueError("a cloud source must hold 3 n float32 values")
            n = points.size() // 3
        else:
            points = _f32(points, (-1, 3))
            n = len(points)
        if not 0 <= offset_points < max(n, 1):
            raise ValueError(f"a cloud of {n} points has no point {offset_points}")
        return cls(SRC_CLOUD, points, T, n_points=n - offset_points, offset_bytes=offset_points * 12)

    def desc(self, data_ptr: int) -> ReprojectSourceDesc:
        fx, fy, cx, cy = self.pinhole
        return ReprojectSourceDesc(data_ptr + self.offset_bytes, self.n_points, self.kind, self.width, self.height, 0, fx, fy, cx, cy, (C.c_float * 16)(*self.T))


def _reproject_counts(cnt: ReprojectCounts, n_sources: int) -> dict:
    per = [dict(samples=s.samples, invalid=s.invalid, range=s.range, outside=s.outside, drawn=s.drawn, won=s.won) for s in list(cnt.source)[:n_sources]]
    return dict(sources=per, covered=cnt.covered, hidden=cnt.hidden, kept=cnt.kept)


def _reproject_table(sources, on_device: bool):
    """(the pr_reproject_source table, what its pointers point into)"""
    srcs = list(sources)
    if not 1 <= len(srcs) <= REPROJECT_MAX_SOURCES or not all(isinstance(s, ReprojectSource) for s in srcs):
        raise ValueError(f"depth_reproject takes 1 .. {REPROJECT_MAX_SOURCES} ReprojectSource objects")
    table, keep = (ReprojectSourceDesc * len(srcs))(), []
    for i, s in enumerate(srcs):
        if on_device:
            dev = s.data if isinstance(s.data, DeviceVector) else DeviceVector.from_host(np.ascontiguousarray(s.data).reshape(-1))
            keep.append(dev)
            table[i] = s.desc(dev.data())
        else:
            if isinstance(s.data, DeviceVector):
                raise ValueError("depth_reproject_host takes host arrays")
            arr = np.ascontiguousarray(s.data)
            keep.append(arr)
            table[i] = s.desc(ptr(arr))
    return table, keep


def depth_reproject(sources, width: int, height: int, K, dtype=np.uint16, params: Optional[ReprojectParamsDesc] = None, depth_out: Optional[DeviceVector] = None,
                    want_source: bool = False, **kw):
    """``pr_depth_reproject_dev``: 1 .. ``REPROJECT_MAX_SOURCES`` sources -- depth frames of other cameras and bare clouds (``ReprojectSource``) --
    through their rigid transforms and the pinhole ``K`` into the z-buffered ``width`` x ``height`` depth frame of one target camera.  Returns (depth
    DeviceVector of ``dtype``[, source DeviceVector uint8[width * height]], counts): ``source`` (``want_source``) holds, per pixel, the index of the
    source that won it, ``REPROJECT_HIDDEN`` or ``REPROJECT_NONE``; ``counts`` is a dict of the per-source records (samples, invalid, range, outside,
    drawn, won) and the frame's covered, hidden and kept pixels.  The frame goes as it is into ``depth_filter`` (whose fill closes rounding gaps
    and hidden pixels), ``init_Scene_projective_device``, ``scene_planes``, ``scene_segments`` and the scorers.  Parameters: a ``ReprojectParams`` or
    its keywords."""
    rp = _params(params, kw, ReprojectParams)
    dt = np.dtype(dtype)
    if dt not in (np.uint16, np.int32):
        raise ValueError("the target depth must be CV_16U or CV_32S")
    table, keep = _reproject_table(sources, True)
    out = _depth_out(depth_out, width * height, dt)
    src = DeviceVector(width * height, np.uint8) if want_source else None
    cnt = ReprojectCounts()
    fx, fy, cx, cy = _pinhole(K)
    check(_lib.load().pr_depth_reproject_dev(C.addressof(table), len(table), width, height, fx, fy, cx, cy, int(dt == np.int32), C.addressof(rp), out.data(),
                                             src.data() if want_source else None, C.addressof(cnt)))
    del keep
    return _with_extras((out,), ((want_source, src),), (_reproject_counts(cnt, len(table)),))


def depth_reproject_host(sources, width: int, height: int, K, dtype=np.uint16, params: Optional[ReprojectParamsDesc] = None, want_source: bool = False, **kw):
    """``pr_depth_reproject_host``: ``depth_reproject`` over host arrays, on the CPU, from the same definition.  Returns (depth[height, width][,
    source uint8[height, width]], counts); runs without a GPU."""
    rp = _params(params, kw, ReprojectParams)
    dt = np.dtype(dtype)
    if dt not in (np.uint16, np.int32):
        raise ValueError("the target depth must be CV_16U or CV_32S")
    table, keep = _reproject_table(sources, False)
    out = np.zeros((height, width), dt)
    src = np.zeros((height, width), np.uint8) if want_source else None
    cnt = ReprojectCounts()
    fx, fy, cx, cy = _pinhole(K)
    check(_lib.load().pr_depth_reproject_host(C.addressof(table), len(table), width, height, fx, fy, cx, cy, int(dt == np.int32), C.addressof(rp), ptr(out),
                                              ptr(src) if want_source else None, C.addressof(cnt)))
    del keep
    return _with_extras((out,), ((want_source, src),), (_reproject_counts(cnt, len(table)),))


def cloud_to_depth(points, width: int, height: int, K, T=None, **kw):
    """``depth_reproject`` of one cloud source: the depth frame a camera with intrinsics ``K`` at ``T`` (cloud to camera) sees of a bare cloud --
    what an ``init_Scene_nn_cloud`` user hands to the scorers, ``scene_planes`` and ``scene_segments``.  Keywords and results as ``depth_reproject``."""
    return depth_reproject([ReprojectSource.cloud(points, T)], width, height, K, **kw)


# ------------------------------------------------------------------------------------------------
# contour check: do the depth edges of a render lie on depth edges of the scene?
# ------------------------------------------------------------------------------------------------
def scene_edge_distance(scene_depth, width: int, height: int, jump_mm: int, radius: int) -> DeviceVector:
    """``pr_scene_edge_distance_dev``: the chessboard distance of every frame pixel to the nearest scene depth edge (the nearer side of a
    jump of more than ``jump_mm``, or of a border to "no measurement"), one uint8 per pixel, 255 where none lies within ``radius``
    (at most ``CONTOUR_MAX_RADIUS``).  ``scene_depth`` as in ``score_poses``.  Made once per frame and handed to ``score_contours``."""
    sd = _scene_depth_dev(scene_depth, width, height)
    out = DeviceVector(width * height, np.uint8)
    check(_lib.load().pr_scene_edge_distance_dev(sd.data(), int(sd.dtype == np.int32), width, height, int(jump_mm), int(radius), out.data()))
    return out


def _edge_dist_dev(edge_dist, width: int, height: int) -> DeviceVector:
    if not isinstance(edge_dist, DeviceVector) or edge_dist.dtype != np.uint8:
        raise ValueError("edge_dist must be the DeviceVector(uint8) that scene_edge_distance returns")
    if edge_dist.size() != width * height:
        raise ValueError(f"edge_dist holds {edge_dist.size()} values, expected {width} x {height}")
    return edge_dist


def _score_contours(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, jump_mm: int, edge_dist, roi, want_overlap: bool):
    call, n = _score_call("pr_score_contours", mesh, width, height, proj, scene_depth, tau_mm, roi)
    ed = _edge_dist_dev(edge_dist, width, height)
    out, con = np.zeros(n, SCORE), np.zeros(n, CONTOUR)
    ov = np.zeros((n, n), np.uint32) if want_overlap else None
    call(int(jump_mm), ed.data(), ptr(out), ptr(con), ptr(ov) if want_overlap else None)
    return (out, con, ov) if want_overlap else (out, con)


def score_contours(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, jump_mm: int, edge_dist,
                   roi: Sequence[int] = (0, 0, 0, 0), want_overlap: bool = False):
    """``pr_score_contours``: one render per pose serves ``score_poses``' records, the contour records and, with ``want_overlap``,
    ``score_overlap``'s matrix.  ``edge_dist`` is ``scene_edge_distance``'s result for the same frame.  Returns (SCORE[P], CONTOUR[P]) or
    (SCORE[P], CONTOUR[P], uint32[P, P]): per hypothesis the edge pixels of its render (``contour``), those within the distance image's
    radius of a scene edge (``hit``, with ``dist_sum`` the sum of their distances), those behind scene surface (``occluded``), the rest (``miss``)."""
    return _score_contours(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, jump_mm, edge_dist, roi, want_overlap)


def score_contours_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int, jump_mm: int, edge_dist,
                         roi: Sequence[int] = (0, 0, 0, 0), want_overlap: bool = False):
    """``pr_score_contours_multi``: ``score_contours`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; everything in pose order."""
    return _score_contours(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, jump_mm, edge_dist, roi, want_overlap)


def contour_fraction(contours) -> np.ndarray:
    """``hit / (contour - occluded)`` in float64: the share of a render's contour, where one can be expected, that lies near a scene edge.
    0 where that denominator is 0 (nothing rendered, or only occluded contour)."""
    c = np.asarray(contours)
    den = c["contour"].astype(np.int64) - c["occluded"].astype(np.int64)
    return np.where(den <= 0, 0.0, c["hit"].astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))


def filter_by_contour(order, contours, min_fraction: float) -> np.ndarray:
    """``order`` (indices, best first, e.g. ``rank_hypotheses(scores)``) without the hypotheses whose ``contour_fraction`` is below
    ``min_fraction``; what remains keeps its order and goes to ``select_hypotheses(order=...)``.  The ranking itself is untouched."""
    order = np.asarray(order, np.int64)
    return order[contour_fraction(contours)[order] >= float(min_fraction)]


# ------------------------------------------------------------------------------------------------
# normal agreement: does the render's surface face the way the scene's does, where their depths agree?
# ------------------------------------------------------------------------------------------------
def _score_normals(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, K, step: int, jump_mm: int, cos_min: float, roi, want_overlap: bool):
    call, n = _score_call("pr_score_normals", mesh, width, height, proj, scene_depth, tau_mm, roi)
    k = _f32(K, -1)
    if k.size != 9:
        raise ValueError("K must hold 9 values")
    out, nrm = np.zeros(n, SCORE), np.zeros(n, NORMAL)
    ov = np.zeros((n, n), np.uint32) if want_overlap else None
    call(ptr(k), int(step), int(jump_mm), float(cos_min), ptr(out), ptr(nrm), ptr(ov) if want_overlap else None)
    return (out, nrm, ov) if want_overlap else (out, nrm)


def score_normals(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, K, step: int, jump_mm: int, cos_min: float,
                  roi: Sequence[int] = (0, 0, 0, 0), want_overlap: bool = False):
    """``pr_score_normals``: one render per pose serves ``score_poses``' records, the normal records and, with ``want_overlap``,
    ``score_overlap``'s matrix.  On every inlier pixel the normal of the render and that of the scene, both estimated from depth by central
    differences over ``step`` pixels (1 .. ``NORMAL_MAX_STEP``) from neighbours within ``jump_mm`` of the centre, agree when the angle
    between them has a cosine of at least ``cos_min``.  Returns (SCORE[P], NORMAL[P]) or (SCORE[P], NORMAL[P], uint32[P, P]): per hypothesis
    the inlier pixels where both normals exist (``tested`` = ``agree`` + ``disagree``) and those where the render's (``no_render_normal``)
    or only the scene's (``no_scene_normal``) does not."""
    return _score_normals(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, K, step, jump_mm, cos_min, roi, want_overlap)


def score_normals_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int, K, step: int, jump_mm: int,
                        cos_min: float, roi: Sequence[int] = (0, 0, 0, 0), want_overlap: bool = False):
    """``pr_score_normals_multi``: ``score_normals`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; everything in pose order."""
    return _score_normals(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, K, step, jump_mm, cos_min, roi, want_overlap)


def normal_fraction(normals) -> np.ndarray:
    """``agree / tested`` in float64: the share of the inlier pixels with both normals whose normals agree.  0 where ``tested`` is 0."""
    n = np.asarray(normals)
    den = n["tested"].astype(np.int64)
    return np.where(den == 0, 0.0, n["agree"].astype(np.float64) / np.where(den == 0, 1, den).astype(np.float64))


def filter_by_normals(order, normals, min_fraction: float) -> np.ndarray:
    """``order`` (indices, best first, e.g. ``rank_hypotheses(scores)``) without the hypotheses whose ``normal_fraction`` is below
    ``min_fraction``; what remains keeps its order and goes to ``select_hypotheses(order=...)``.  The ranking itself is untouched."""
    order = np.asarray(order, np.int64)
    return order[normal_fraction(normals)[order] >= float(min_fraction)]


# ------------------------------------------------------------------------------------------------
# pose observability: the information matrix of a hypothesis and its eigenvectors
# ------------------------------------------------------------------------------------------------
def _robust_ptr(robust: Optional["Robust"]):
    if robust is not None and not isinstance(robust, Robust):
        raise ValueError("robust: a Robust or None")
    return C.addressof(robust.desc()) if robust is not None else None


def icp_information(clouds: DeviceVector, offsets, scene, centers, radii, robust: Optional[Robust] = None, want_eig: bool = True, packed: bool = False):
    """``pr_icp_information``: for each cloud (``offsets``: P + 1 point offsets into ``clouds``) the float64 sums of the weighted point-to-plane
    normal system about ``centers[i]`` with the rotational half scaled by ``radii[i]`` (metres, camera frame), and their eigen-decomposition.
    Returns (info[P] of POSE_INFO dtype, eig[P] of POSE_EIG dtype or None).  The clouds are not modified.  ``packed``: the audit form, which
    reads a projective scene through its packed record (``pr_debug_icp_information``)."""
    offsets = np.ascontiguousarray(offsets, np.uint32)
    if len(offsets) == 0:
        raise ValueError("offsets: P + 1 point offsets (at least one)")
    if int(offsets[-1]) * 3 > clouds.size():
        raise ValueError(f"offsets end at point {int(offsets[-1])}, the cloud buffer holds {clouds.size() // 3}")
    n = len(offsets) - 1
    c, r = _f32(centers, (-1, 3)), _f32(radii, -1)
    if len(c) != n or len(r) != n:
        raise ValueError(f"centers and radii: one per cloud ({n}), got {len(c)} and {len(r)}")
    info = np.zeros(n, _lib.POSE_INFO)
    eig = np.zeros(n, _lib.POSE_EIG) if want_eig else None
    d = scene.desc()
    tail = (_robust_ptr(robust), ptr(c), ptr(r), ptr(info), ptr(eig) if want_eig else None)
    if packed:
        check(_lib.load().pr_debug_icp_information(clouds.data() or None, ptr(offsets), n, scene.kind, C.addressof(d), 1, *tail))
    else:
        check(_lib.load().pr_icp_information(clouds.data() or None, ptr(offsets), n, scene.kind, C.addressof(d), *tail))
    return info, eig


def _model_center_radius(tris, center, radius):
    """``center`` (model frame and units) and ``radius`` (metres) of one mesh: given, or -- a ``Model`` -- the midpoint of its bounding box and
    half the box diagonal (millimetres, hence / 1000)."""
    if center is None or radius is None:
        if not isinstance(tris, Model):
            raise ValueError("center and radius default only for a Model (its bounding box); give both for a triangle array")
        lo, hi = np.asarray(tris.bbox_min, np.float64), np.asarray(tris.bbox_max, np.float64)
        if center is None:
            center = 0.5 * (lo + hi)
        if radius is None:
            radius = 0.5 * float(np.linalg.norm(hi - lo)) / 1000.0
    return _f32(center, 3), float(radius)


def pose_information(tris, poses, width: int, height: int, proj, K, scene, center=None, radius=None, roi: Optional[Sequence[int]] = None,
                     robust: Optional[Robust] = None, want_eig: bool = True):
    """``pr_pose_information``: ``refine_batch``'s render and clouds, then the information pass: how well the scene constrains each hypothesis.
    ``center`` (model frame, model units) is moved by each pose; ``radius`` is in metres.  For a ``Model`` they default to the midpoint of
    ``bbox_min`` / ``bbox_max`` and half the box diagonal.  Returns (info[P], eig[P] or None, cloud sizes[P])."""
    cm, rad = _model_center_radius(tris, center, radius)
    td = _tris_dev(tris)
    poses = _f32(poses, (-1, 16))
    pj, k = _f32(proj, -1), _f32(K, -1)
    n = len(poses)
    info, sizes = np.zeros(n, _lib.POSE_INFO), np.zeros(n, np.uint32)
    eig = np.zeros(n, _lib.POSE_EIG) if want_eig else None
    d = scene.desc()
    check(_lib.load().pr_pose_information(td.data() or None, td.size() // 9, ptr(poses), n, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                          Roi(*(roi if roi is not None else (0, 0, 0, 0))), _robust_ptr(robust), ptr(cm), rad, ptr(info),
                                          ptr(eig) if want_eig else None, ptr(sizes)))
    return info, eig, sizes


def pose_information_multi(meshes, mesh_index, poses, width: int, height: int, proj, K, scene, centers=None, radii=None,
                           roi: Optional[Sequence[int]] = None, robust: Optional[Robust] = None, want_eig: bool = True):
    """``pr_pose_information_multi``: ``pose_information`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; ``centers`` / ``radii``: one per
    mesh (None: each ``Model``'s defaults).  Every record equals the single-mesh call's."""
    meshes = list(meshes)
    cr = [_model_center_radius(m, None if centers is None else centers[i], None if radii is None else radii[i]) for i, m in enumerate(meshes)]
    cm = _f32([c for c, _ in cr], (-1, 3)) if cr else np.zeros((1, 3), np.float32)
    rad = _f32([r for _, r in cr], -1) if cr else np.ones(1, np.float32)
    table, devs, idx, poses = _multi_inputs(meshes, mesh_index, poses)
    pj, k = _f32(proj, -1), _f32(K, -1)
    n = len(poses)
    info, sizes = np.zeros(n, _lib.POSE_INFO), np.zeros(n, np.uint32)
    eig = np.zeros(n, _lib.POSE_EIG) if want_eig else None
    d = scene.desc()
    check(_lib.load().pr_pose_information_multi(table, len(devs), ptr(idx), ptr(poses), n, width, height, ptr(pj), ptr(k), scene.kind, C.addressof(d),
                                                Roi(*(roi if roi is not None else (0, 0, 0, 0))), _robust_ptr(robust), ptr(cm), ptr(rad), ptr(info),
                                                ptr(eig) if want_eig else None, ptr(sizes)))
    return info, eig, sizes


def _sym6(v21) -> np.ndarray:
    m = np.zeros((6, 6))
    m[np.triu_indices(6)] = np.asarray(v21, np.float64)
    return m + np.triu(m, 1).T


def information_matrix(info) -> np.ndarray:
    """The symmetric 6 x 6 of one POSE_INFO record (``H`` holds its upper triangle, row-major)."""
    return _sym6(info["H"])


def pose_covariance(info, eig, min_ratio: float, sigma: Optional[float] = None, physical: bool = True):
    """``pr_info_covariance`` for one record pair: (cov 6 x 6, rank, sigma2).  Eigenpairs with ``lambda <= min_ratio * lambda[5]`` (or
    ``lambda <= 0``) are left out: the covariance is that of the observable directions alone.  ``sigma`` (metres): the sensor's standard
    deviation; None: the residual variance ``(sum_wr2 / sum_w) * n_valid / (n_valid - 6)``.  ``physical``: rotational rows and columns divided
    by ``rho`` -- radians and metres -- instead of the scaled coordinates of the record."""
    i, e = np.ascontiguousarray(info, _lib.POSE_INFO).reshape(1), np.ascontiguousarray(eig, _lib.POSE_EIG).reshape(1)
    cov = np.zeros(21, np.float64)
    rank, s2 = C.c_uint32(), C.c_double()
    check(_lib.load().pr_info_covariance(ptr(i), ptr(e), float(sigma) if sigma is not None else 0.0, float(min_ratio), ptr(cov), C.byref(rank), C.byref(s2)))
    m = _sym6(cov)
    if physical:
        sc = np.array([1.0 / float(i["rho"][0])] * 3 + [1.0] * 3)
        m = m * sc[:, None] * sc[None, :]
    return m, int(rank.value), float(s2.value)


def observable_rank(eig, min_ratio: float) -> np.ndarray:
    """Per POSE_EIG record the number of k with ``lambda[k] > 0`` and ``lambda[k] > min_ratio * lambda[5]`` (``pr_info_covariance``'s rank)."""
    lam = np.asarray(eig)["lambda"].reshape(-1, 6)
    return ((lam > 0.0) & (lam > float(min_ratio) * lam[:, 5:6])).sum(1)


def weakest_twist(info, eig, k: int = 0):
    """Eigenvector ``k`` (0: the least constrained motion) of one record pair as a twist about the record's centre: (omega in radians, t in
    metres), i.e. the rotational half divided by ``rho``."""
    v = np.asarray(eig["V"], np.float64).reshape(6, 6)[:, int(k)]
    return v[:3] / float(np.asarray(info["rho"]).reshape(-1)[0]), v[3:].copy()


def filter_by_observability(order, eig, min_ratio: float, min_rank: int = 6) -> np.ndarray:
    """``order`` (indices, best first) without the hypotheses whose ``observable_rank(eig, min_ratio)`` is below ``min_rank``; what remains keeps
    its order.  The ranking itself is untouched."""
    order = np.asarray(order, np.int64)
    return order[observable_rank(eig, min_ratio)[order] >= int(min_rank)]


# ------------------------------------------------------------------------------------------------
# contour alignment: the silhouette's normal equations, and a pose step along the observable directions
# ------------------------------------------------------------------------------------------------
def scene_edge_nearest(scene_depth, width: int, height: int, jump_mm: int, radius: int) -> DeviceVector:
    """``pr_scene_edge_nearest_dev``: for every frame pixel the nearest scene depth edge pixel (``scene_edge_distance``'s edge pixels) within
    the (2 radius + 1)^2 window around it as ``ey << 16 | ex``, ``EDGE_NONE`` where the window holds none; ties go to the smaller squared
    distance, then the smaller ey, then the smaller ex.  One uint32 per pixel.  Made once per frame and handed to ``contour_information``."""
    sd = _scene_depth_dev(scene_depth, width, height)
    out = DeviceVector(width * height, np.uint32)
    check(_lib.load().pr_scene_edge_nearest_dev(sd.data(), int(sd.dtype == np.int32), width, height, int(jump_mm), int(radius), out.data()))
    return out


def _nearest_dev(nearest, width: int, height: int) -> DeviceVector:
    if not isinstance(nearest, DeviceVector) or nearest.dtype != np.uint32:
        raise ValueError("nearest must be the DeviceVector(uint32) that scene_edge_nearest returns")
    if nearest.size() != width * height:
        raise ValueError(f"nearest holds {nearest.size()} values, expected {width} x {height}")
    return nearest


def _contour_information(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, jump_mm: int, nearest, K, cm, rad, roi, want_scores: bool):
    call, n = _score_call("pr_contour_information", mesh, width, height, proj, scene_depth, tau_mm, roi if roi is not None else (0, 0, 0, 0))
    nd = _nearest_dev(nearest, width, height)
    k = _f32(K, -1)
    if k.size != 9:
        raise ValueError("K must hold 9 values")
    scores = np.zeros(n, SCORE) if want_scores else None
    fit, info = np.zeros(n, CONTOUR_FIT), np.zeros(n, _lib.POSE_INFO)
    call(int(jump_mm), nd.data(), ptr(k), ptr(cm), rad if isinstance(rad, float) else ptr(rad),      # (one mesh: the radius by value; a table: one per mesh)
         ptr(scores) if want_scores else None, ptr(fit), ptr(info))
    return scores, fit, info


def contour_information(tris, poses, width: int, height: int, proj, K, scene_depth, tau_mm: int, jump_mm: int, nearest, center=None, radius=None,
                        roi: Optional[Sequence[int]] = None, want_scores: bool = True):
    """``pr_contour_information``: one render per pose; every edge pixel of the render that is not occluded and has a scene edge pixel in
    ``nearest`` (``scene_edge_nearest``'s map of the same frame) contributes the two rows of its pixel offset, in metres at its depth, to a
    float64 information record about the pose's centre -- the coordinates of ``pose_information`` (same ``center`` / ``radius`` defaults), so
    the two records can go to ``combine_information``.  Returns (SCORE[P] or None, CONTOUR_FIT[P], POSE_INFO[P])."""
    cm, rad = _model_center_radius(tris, center, radius)
    return _contour_information(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, jump_mm, nearest, K, cm, rad, roi, want_scores)


def contour_information_multi(meshes, mesh_index, poses, width: int, height: int, proj, K, scene_depth, tau_mm: int, jump_mm: int, nearest,
                              centers=None, radii=None, roi: Optional[Sequence[int]] = None, want_scores: bool = True):
    """``pr_contour_information_multi``: ``contour_information`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; ``centers`` / ``radii``:
    one per mesh (None: each ``Model``'s defaults).  Every record equals the single-mesh call's."""
    meshes = list(meshes)
    cm, rad = _mesh_centers_radii(meshes, centers, radii)
    return _contour_information(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, jump_mm, nearest, K, cm, rad, roi, want_scores)


def _mesh_centers_radii(meshes, centers, radii):
    cr = [_model_center_radius(m, None if centers is None else centers[i], None if radii is None else radii[i]) for i, m in enumerate(meshes)]
    cm = _f32([c for c, _ in cr], (-1, 3)) if cr else np.zeros((1, 3), np.float32)
    rad = _f32([r for _, r in cr], -1) if cr else np.ones(1, np.float32)
    return cm, rad


def combine_information(a, b, wa: float = 1.0, wb: float = 1.0) -> np.ndarray:
    """``pr_info_combine`` record by record (host only): ``wa * a + wb * b`` for H, g, sum_w and sum_wr2; sum_r2 and the counts are added.  The
    records of a pair must be about the same centre and radius, bit for bit."""
    a, b = np.ascontiguousarray(a, _lib.POSE_INFO).reshape(-1), np.ascontiguousarray(b, _lib.POSE_INFO).reshape(-1)
    if len(a) != len(b):
        raise ValueError(f"combine_information: {len(a)} records against {len(b)}")
    out = np.zeros(len(a), _lib.POSE_INFO)
    lib, sz = _lib.load(), _lib.POSE_INFO.itemsize
    for i in range(len(a)):
        check(lib.pr_info_combine(ptr(a) + i * sz, float(wa), ptr(b) + i * sz, float(wb), ptr(out) + i * sz))
    return out


def information_eig(info) -> np.ndarray:
    """``pr_info_eig`` record by record (host only): the cyclic Jacobi of ``pose_information``'s eigen kernel, on the host.  POSE_EIG[P]."""
    info = np.ascontiguousarray(info, _lib.POSE_INFO).reshape(-1)
    out = np.zeros(len(info), _lib.POSE_EIG)
    lib = _lib.load()
    for i in range(len(info)):
        check(lib.pr_info_eig(ptr(info) + i * _lib.POSE_INFO.itemsize, ptr(out) + i * _lib.POSE_EIG.itemsize))
    return out


def information_step(info, eig, poses, min_ratio: float):
    """``pr_info_step`` record by record (host only): every pose moved by the solution of ``H delta = g`` restricted to the eigenpairs
    ``observable_rank`` counts -- a twist about the record's centre, rotational half divided by ``rho``.  Returns (poses float32[P, 4, 4],
    delta float64[P, 6], rank int64[P]); a record of rank 0 leaves its pose as it is."""
    info = np.ascontiguousarray(info, _lib.POSE_INFO).reshape(-1)
    eig = np.ascontiguousarray(eig, _lib.POSE_EIG).reshape(-1)
    pin = _f32(poses, (-1, 16))
    if not (len(info) == len(eig) == len(pin)):
        raise ValueError(f"information_step: {len(info)} info records, {len(eig)} eig records, {len(pin)} poses")
    out, delta, rank = np.zeros_like(pin), np.zeros((len(pin), 6), np.float64), np.zeros(len(pin), np.int64)
    lib, r = _lib.load(), C.c_uint32()
    for i in range(len(pin)):
        check(lib.pr_info_step(ptr(info) + i * _lib.POSE_INFO.itemsize, ptr(eig) + i * _lib.POSE_EIG.itemsize, float(min_ratio), ptr(pin) + i * 64,
                               ptr(out) + i * 64, ptr(delta) + i * 48, C.byref(r)))
        rank[i] = r.value
    return out.reshape(-1, 4, 4), delta, rank


def _refine_contours(surface, contour, poses, iterations: int, weight: float, min_ratio: float, min_used: int):
    """The loop of ``refine_contours``: surface(poses) -> POSE_INFO[P], contour(poses) -> (CONTOUR_FIT[P], POSE_INFO[P])."""
    poses = _f32(poses, (-1, 16)).reshape(-1, 4, 4).copy()
    n, iters = len(poses), int(iterations)
    live = np.ones(n, bool)
    hist = dict(rank=np.zeros((iters, n), np.int64), used=np.zeros((iters, n), np.int64), rms_px=np.full((iters, n), np.nan))
    for it in range(iters):
        surf = surface(poses)
        fit, con = contour(poses)
        both = combine_information(surf, con, 1.0, weight)
        eig = information_eig(both)
        stepped, _, rank = information_step(both, eig, poses, min_ratio)
        live &= (fit["used"] >= int(min_used)) & (surf["n_valid"] > 0)
        poses[live] = stepped[live]
        used = fit["used"].astype(np.int64)
        hist["rank"][it], hist["used"][it] = rank, used
        hist["rms_px"][it] = np.where(used > 0, np.sqrt(fit["sum_d2"].astype(np.float64) / np.maximum(used, 1)), np.nan)
    return poses, hist


def refine_contours(tris, poses, width: int, height: int, proj, K, scene, scene_depth, nearest, tau_mm: int, jump_mm: int, *, iterations: int,
                    weight: float, min_ratio: float, min_used: int, center=None, radius=None, roi: Optional[Sequence[int]] = None,
                    robust: Optional[Robust] = None):
    """Pose steps on the surface and the silhouette together.  Per iteration: ``pose_information`` (``scene``, ``robust``) and
    ``contour_information`` (``scene_depth``, ``nearest``) at the current poses, ``combine_information(1, weight)``, ``information_eig`` and
    ``information_step(min_ratio)``: the silhouette pins the motions the surface leaves free, and what neither constrains is not stepped along.
    A hypothesis with fewer than ``min_used`` used contour pixels, or without a surface correspondence, keeps its pose from then on.  Returns
    (poses float32[P, 4, 4], history) with ``history["rank"]``, ``["used"]`` and ``["rms_px"]`` (sqrt(sum_d2 / used), the contour's RMS pixel
    distance; nan without used pixels) of shape (iterations, P), each as found BEFORE that iteration's step."""
    cm, rad = _model_center_radius(tris, center, radius)
    return _refine_contours(
        lambda p: pose_information(tris, p, width, height, proj, K, scene, cm, rad, roi, robust, want_eig=False)[0],
        lambda p: contour_information(tris, p, width, height, proj, K, scene_depth, tau_mm, jump_mm, nearest, cm, rad, roi, want_scores=False)[1:],
        poses, iterations, weight, min_ratio, min_used)


def refine_contours_multi(meshes, mesh_index, poses, width: int, height: int, proj, K, scene, scene_depth, nearest, tau_mm: int, jump_mm: int, *,
                          iterations: int, weight: float, min_ratio: float, min_used: int, centers=None, radii=None,
                          roi: Optional[Sequence[int]] = None, robust: Optional[Robust] = None):
    """``refine_contours`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; ``centers`` / ``radii``: one per mesh."""
    meshes = list(meshes)
    cm, rad = _mesh_centers_radii(meshes, centers, radii)
    return _refine_contours(
        lambda p: pose_information_multi(meshes, mesh_index, p, width, height, proj, K, scene, cm, rad, roi, robust, want_eig=False)[0],
        lambda p: contour_information_multi(meshes, mesh_index, p, width, height, proj, K, scene_depth, tau_mm, jump_mm, nearest, cm, rad, roi,
                                            want_scores=False)[1:],
        poses, iterations, weight, min_ratio, min_used)


# ------------------------------------------------------------------------------------------------
# composition: the detections of a frame taken together
# ------------------------------------------------------------------------------------------------
def _compose_detections(mesh, width: int, height: int, proj, scene_depth, tau_mm: int, roi, want_labels: bool, want_depth: bool):
    call, n = _score_call("pr_compose_detections", mesh, width, height, proj, scene_depth, tau_mm, roi)
    labels = DeviceVector(width * height, np.uint16) if want_labels and n else None
    depth = DeviceVector(width * height, np.int32) if want_depth and n else None    # (a call without hypotheses writes nothing: no frames then)
    out, vis, frame = np.zeros(n, SCORE), np.zeros(n, VISIBLE), np.zeros(1, FRAME)
    call(labels.data() if labels else None, depth.data() if depth else None, ptr(out), ptr(vis), ptr(frame))
    return labels, depth, out, vis, frame[0]


def compose_detections(tris, poses, width: int, height: int, proj, scene_depth, tau_mm: int, roi: Sequence[int] = (0, 0, 0, 0),
                       want_labels: bool = True, want_depth: bool = True):
    """``pr_compose_detections``: the poses -- typically ``select_hypotheses``' detections -- rendered into one frame.  Returns
    (labels, depth, scores, visible, frame): ``labels`` a DeviceVector(uint16) of width x height with, per frame pixel, the index of the
    hypothesis whose render is in front there (the lowest index on a tie) or ``COMPOSE_NONE``; ``depth`` a DeviceVector(int32) with that
    front depth or 0 (each None when not wanted, or when there are no poses); ``scores`` = ``score_poses``' bytes; ``visible`` =
    VISIBLE[P], the pixels every hypothesis owns by the four tests; ``frame`` = one FRAME record of the frame against the composite.
    At most ``COMPOSE_MAX_POSES`` hypotheses per call."""
    return _compose_detections(_one_mesh(tris, poses), width, height, proj, scene_depth, tau_mm, roi, want_labels, want_depth)


def compose_detections_multi(meshes, mesh_index, poses, width: int, height: int, proj, scene_depth, tau_mm: int,
                             roi: Sequence[int] = (0, 0, 0, 0), want_labels: bool = True, want_depth: bool = True):
    """``pr_compose_detections_multi``: ``compose_detections`` for a batch whose pose i uses ``meshes[mesh_index[i]]``; labels, ties and
    records in pose order."""
    return _compose_detections(_mesh_batch(meshes, mesh_index, poses), width, height, proj, scene_depth, tau_mm, roi, want_labels, want_depth)


def visible_fraction(scores, visible) -> np.ndarray:
    """``owned / visible`` in float64: the share of a hypothesis' render that no other hypothesis of the composed set hides.  0 where
    nothing is visible."""
    sc, vi = np.asarray(scores), np.asarray(visible)
    den = sc["visible"].astype(np.int64)
    return np.where(den <= 0, 0.0, vi["owned"].astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))


def rank_hypotheses_per_mesh(scores, mesh_index) -> dict:
    """``rank_hypotheses`` within each mesh of a mixed batch: {mesh: indices into the whole batch, best first}.  Only meshes that have
    hypotheses appear."""
    sc = np.asarray(scores)
    idx = np.asarray(mesh_index)
    if idx.ndim != 1 or len(idx) != len(sc):
        raise ValueError(f"mesh_index must hold one entry per score: got shape {idx.shape} for {len(sc)} scores")
    out = {}
    for m in np.unique(idx):
        members = np.flatnonzero(idx == m)
        out[int(m)] = members[rank_hypotheses(sc[members])]
    return out


def eigen_slover_666(A, b) -> np.ndarray:
    """``cuda_icp::eigen_slover_666`` (icp.cpp:29-45, public in icp.h:54)."""
    T = np.zeros(16, np.float32)
    a, bb = _f32(A, -1), _f32(b, -1)
    _lib.load().pr_solve_666(ptr(a), ptr(bb), ptr(T))
    return T.reshape(4, 4)
