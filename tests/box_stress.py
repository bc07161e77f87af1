"""Hard cases for the per-hypothesis pixel boxes -- TEST INFRASTRUCTURE (numpy and the CPU oracle only, no device).

Every hot path rasterises into a pixel box per hypothesis: the loose one (pose_pixel_box, csrc/pose_box.h: the hull of the eight projected
corners of the mesh's box plus 2 pixels) or the tight one (tight_pixel_box: the hull of the projected vertices).  A box that is too small
faults nothing: it clips a pixel and silently changes a cloud, a score or a label.  This module makes the poses that press on the boxes --
strong perspective, every frame border, exotic intrinsics, mesh coordinates far from the origin, boxes of a few pixels, needles, nothing at
all -- on a 160 x 120 frame, with the oracle's FULL-FRAME renders of them (oracle_lib.render knows no boxes) as the reference everything is
held to.  Deterministic: fixed seeds, and `assert_classes` states what the committed seeds must yield.

Also the helpers test_tight_box.py introduced (area, inside, drawn_box, numpy_tight_box), which both host files import from here, and what
the references of the pair kernels and the contour fit (solid_ref, vsd_ref, select_ref, contour_fit_ref: they take renders and know no
boxes either) give on the same batches, computed once, with `assert_pair_classes` for what those must contain."""
import functools

import numpy as np

import oracle_lib as O
from contour_fit_ref import centers, fit_records, nearest_ref
from gpu_common import random_mesh, random_pose
from pose_refine_amd import api
from select_ref import overlap_ref
from solid_ref import INT_MAX, INT_MIN, pairs_ref, span_ref
from vsd_ref import SMALL_TAUS, vsd_ref

W, H = 160, 120
NONE = (0, 0, 0, 0)
ROIS = [(30, 20, 91, 71), (70, 50, 37, 23)]                       # two windows that cut the silhouettes; odd sizes, the second narrower than a 64-column strip
f32 = np.float32
TAU = 8
MAX_BATCH = 96


def default_K():
    return np.array([1.1 * W, 0, W / 2, 0, 1.1 * W, H / 2, 0, 0, 1], f32)


# ---- the helpers of test_tight_box.py ---------------------------------------------------------------------------------------------------
def area(b):
    return max(int(b[2]) - int(b[0]) + 1, 0) * max(int(b[3]) - int(b[1]) + 1, 0)


def inside(inner, outer):
    return area(inner) == 0 or (inner[0] >= outer[0] and inner[1] >= outer[1] and inner[2] <= outer[2] and inner[3] <= outer[3])


def box_of_image(img, height, roi=NONE):
    """{x0, y0, x1, y1} in RASTER coordinates (row flipped back) of the non-zero pixels of one of the oracle's renders (with a ROI: the
    window's image), or None."""
    rows, cols = np.nonzero(img)
    if len(rows) == 0:
        return None
    rows = rows + (roi[1] if roi[2] > 0 and roi[3] > 0 else 0)
    cols = cols + (roi[0] if roi[2] > 0 and roi[3] > 0 else 0)
    return np.array([cols.min(), height - 1 - rows.max(), cols.max(), height - 1 - rows.min()])


def drawn_box(tris, pose, proj, roi=NONE, width=W, height=H):
    """box_of_image of the pixels the oracle's raster draws for one pose."""
    return box_of_image(O.render(tris, pose[None], width, height, proj, roi)[0], height, roi)


def numpy_tight_box(tris, pose, proj, loose, width=W, height=H):
    """vertex_to_screen / tight_pixel_box (csrc/pose_box.h) restated in float32 numpy, operation by operation."""
    v = np.ascontiguousarray(tris, f32).reshape(-1, 3)
    M, P = np.asarray(pose, f32).reshape(16), np.asarray(proj, f32).reshape(16)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        lx = M[0] * x + M[1] * y + M[2] * z + M[3]
        ly = M[4] * x + M[5] * y + M[6] * z + M[7]
        lz = M[8] * x + M[9] * y + M[10] * z + M[11]
        cx = P[0] * lx + P[1] * ly + P[2] * lz + P[3]
        cy = P[4] * lx + P[5] * ly + P[6] * lz + P[7]
        px = cx / lz * f32(width) / f32(2) + f32(width) / f32(2)
        py = cy / lz * f32(height) / f32(2) + f32(height) / f32(2)
        bad = np.any(~(lz > f32(1e-3))) or np.any(~(np.abs(px) < f32(1e8))) or np.any(~(np.abs(py) < f32(1e8)))
    if bad or len(v) == 0:
        return np.asarray(loose)
    return np.array([max(loose[0], int(np.floor(px.min())) - 2), max(loose[1], int(np.floor(py.min())) - 2),
                     min(loose[2], int(np.ceil(px.max())) + 2), min(loose[3], int(np.ceil(py.max())) + 2)])


def assert_boxes_hold(tris, pose, proj, image, roi=NONE, width=W, height=H, what=""):
    """The three assertions of the host tests for one hypothesis and the oracle's render of it: tight in loose, the drawn pixels in both, and
    the tight box equal to the numpy restatement.  Returns (tight, loose, drawn)."""
    tight, loose = api.tight_box(tris, pose, width, height, proj, roi)
    drawn = box_of_image(image, height, roi)
    assert inside(tight, loose), (what, tight, loose)
    assert drawn is None or (area(tight) > 0 and area(loose) > 0 and inside(drawn, tight) and inside(drawn, loose)), (what, drawn, tight, loose)
    assert np.array_equal(tight, numpy_tight_box(tris, pose, proj, loose, width, height)), (what, tight, loose)
    return tight, loose, drawn


# ---- the meshes -------------------------------------------------------------------------------------------------------------------------
def soup_mesh():
    return random_mesh(np.random.default_rng(101), 300, 40.0)


def shell_mesh():
    """400 small triangles with every vertex on a sphere of radius 50: the corners of the mesh's box are empty space."""
    rng = np.random.default_rng(102)
    c = rng.normal(size=(400, 1, 3))
    c /= np.linalg.norm(c, axis=2, keepdims=True)
    v = c + rng.normal(size=(400, 3, 3)) * 0.12
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    return np.ascontiguousarray((v * 50.0).astype(f32))


def needle_mesh(width_mm):
    """One triangle 60 mm long and `width_mm` wide."""
    return np.array([[[-30, 0, 0], [30, 0, 0], [0, width_mm, 0]]], f32)


def box_corners(tris):
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)])


def offset_mesh(tris, o):
    return np.ascontiguousarray((np.asarray(tris, np.float64) + np.asarray(o, np.float64)).astype(f32))


# ---- the families: each draws gpu_common.random_pose and modifies it ---------------------------------------------------------------------
def close_pose(rng, tris, use_corners):
    """Pushed along z until the nearest vertex (or corner of the mesh's box) stands eps in front of the camera plane, eps log-uniform in
    10^-2.9 .. 10^1.5 mm; pushed sideways too, so that the silhouette's edge is often inside the frame."""
    p = random_pose(rng, 300.0)
    pts = box_corners(tris) if use_corners else np.asarray(tris, np.float64).reshape(-1, 3)
    eps = 10.0 ** rng.uniform(-2.9, 1.5)
    p[:2, 3] = (rng.normal(size=2) * 45.0).astype(f32)
    p[2, 3] = f32(eps - (pts @ p[2, :3].astype(np.float64)).min())
    return p


def border_pose(rng, axis, sign):
    p = random_pose(rng, 300.0)
    p[:3, 3] = (0.0, 0.0, 300.0 + rng.uniform(-20, 20))
    p[axis, 3] = f32(sign * rng.uniform(60.0, 140.0))
    return p


def corner_pose(rng):
    p = random_pose(rng, 300.0)
    p[:3, 3] = (125.0, -95.0, 300.0)
    return p


def far_pose(rng):
    return random_pose(rng, 10.0 ** rng.uniform(3.0, 5.0))


def nothing_poses(rng):
    behind, aside = random_pose(rng, 300.0), random_pose(rng, 300.0)
    behind[:3, 3] = (0.0, 0.0, -300.0)
    aside[:3, 3] = (4000.0, 0.0, 300.0)
    return [behind, aside]


def straddle_pose(rng):
    """The camera inside the mesh: vertices on both sides of the camera plane, so fragments with negative depth (see drawn_count) beside and
    over surface in front, in a whole-frame box."""
    p = random_pose(rng, 300.0)
    p[:3, 3] = (rng.normal() * 10.0, rng.normal() * 10.0, rng.uniform(5.0, 40.0))
    return p


def exotic_K(rng):
    """Focal length W * 10^u, u in -0.7 .. 1.3; fy / fx in 0.5 .. 2; the principal point displaced by a normal deviate of one frame size."""
    fx = W * 10.0 ** rng.uniform(-0.7, 1.3)
    fy = fx * 2.0 ** rng.uniform(-1.0, 1.0)
    return np.array([fx, 0, W / 2 + rng.normal() * W, 0, fy, H / 2 + rng.normal() * H, 0, 0, 1], f32)


def intrinsics_pose(rng, K):
    """Distance 10^1.8 .. 10^3.5 mm, on the ray through the middle of the frame (the principal point may be far outside it)."""
    d = 10.0 ** rng.uniform(1.8, 3.5)
    p = random_pose(rng, d)
    k = K.astype(np.float64)
    p[:3, 3] = (np.array([(W / 2 - k[2]) / k[0], (H / 2 - k[5]) / k[4], 1.0]) * d + rng.normal(size=3) * d * 0.05).astype(f32)
    return p


def offset_pose(rng, o):
    """The pose that undoes the mesh's offset o: t - R o in float64, then rounded.  Inside M v the two cancel, with the rounding of |o|."""
    p = random_pose(rng, 300.0)
    p[:3, 3] = (p[:3, 3].astype(np.float64) - p[:3, :3].astype(np.float64) @ o).astype(f32)
    return p


def random_offset(rng, exponent):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a) * 10.0 ** exponent


# ---- the batches ------------------------------------------------------------------------------------------------------------------------
def scene_of(renders, rng):
    """As verify_ref.launch_split_case makes its scene: what is in front among the first few renders with +-6 mm noise, 10 % holes, a wall
    behind.  int32, every value within uint16."""
    first = np.asarray(renders[:6]).astype(np.int64)
    front = np.where((first > 0) & (first < 60000), first, 1 << 40).min(0)
    front[front == 1 << 40] = 0
    scene = front + rng.integers(-6, 7, front.shape) * (front > 0)
    scene[(front == 0) & (rng.random(front.shape) < 0.6)] = 700
    scene[rng.random(front.shape) < 0.1] = 0
    scene = np.clip(scene, 0, 65535)
    return np.ascontiguousarray(scene.astype(np.int32))


def _batch(name, tris, K, poses, families, rng, decade=None):
    poses = np.ascontiguousarray(np.stack(poses), f32)
    assert len(poses) <= MAX_BATCH and len(poses) == len(families)
    order = rng.permutation(len(poses))                            # whole-frame, 1-pixel and empty boxes side by side, and in every sub-batch
    poses, families = np.ascontiguousarray(poses[order]), [families[i] for i in order]
    proj = O.compute_proj(K, W, H)
    R = O.render(tris, poses, W, H, proj)
    return dict(name=name, tris=np.ascontiguousarray(tris, f32), K=K, proj=proj, poses=poses, families=families, R=R, scene=scene_of(R, rng),
                decade=decade)


def _mesh_batch(name, tris, seed):
    """close, border, far, nothing and straddle on one mesh with the default intrinsics."""
    rng = np.random.default_rng(seed)
    poses, fam = [], []
    for i in range(36):
        poses.append(close_pose(rng, tris, i % 2 == 1)); fam.append("close")
    for axis in (0, 1):
        for sign in (-1, 1):
            for _ in range(5):
                poses.append(border_pose(rng, axis, sign)); fam.append("border")
    poses.append(corner_pose(rng)); fam.append("border")
    for _ in range(16):
        poses.append(far_pose(rng)); fam.append("far")
    for p in nothing_poses(rng):
        poses.append(p); fam.append("nothing")
    for _ in range(3):
        poses.append(straddle_pose(rng)); fam.append("straddle")
    return _batch(name, tris, default_K(), poses, fam, rng)


OFFSET_EXPONENTS = (3.4, 4.7, 5.2, 6.5, 7.1, 7.45)


@functools.lru_cache(maxsize=None)
def stress_batches():
    """The batches the tests share and leave as they are: a list of dicts with name, tris, K, proj, poses (P, 4, 4), families (a name per
    hypothesis), R (the oracle's full-frame renders), scene (int32, within uint16) and decade (of an offset mesh, else None)."""
    soup, shell = soup_mesh(), shell_mesh()
    out = [_mesh_batch("soup", soup, 1), _mesh_batch("shell", shell, 2)]
    for n, (mesh, e) in enumerate(zip((soup, shell) * 3, OFFSET_EXPONENTS)):
        rng = np.random.default_rng(300 + n)
        o = random_offset(rng, e)
        out.append(_batch(f"offset_1e{e}", offset_mesh(mesh, o), default_K(), [offset_pose(rng, o) for _ in range(8)], ["offset"] * 8, rng,
                          decade=int(np.floor(e))))
    for n, mesh in enumerate((soup, shell, soup, shell, soup, shell)):
        rng = np.random.default_rng(400 + n)
        K = exotic_K(rng)
        out.append(_batch(f"intrinsics_{n}", mesh, K, [intrinsics_pose(rng, K) for _ in range(10)], ["intrinsics"] * 10, rng))
    for n, wd in enumerate((1e-3, 0.03, 1.0)):
        rng = np.random.default_rng(500 + n)
        out.append(_batch(f"needle_{wd}", needle_mesh(wd), default_K(), [random_pose(rng, 300.0) for _ in range(8)], ["needle"] * 8, rng))
    return out


@functools.lru_cache(maxsize=None)
def roi_renders(index, roi):
    """The oracle's renders of batch `index` inside the window `roi`, computed once."""
    b = stress_batches()[index]
    return O.render(b["tris"], b["poses"], W, H, b["proj"], roi)


@functools.lru_cache(maxsize=None)
def batch_boxes(index):
    """(tight[P, 4], loose[P, 4]) of batch `index` from the host twin (api.tight_box, no device)."""
    b = stress_batches()[index]
    t, l = zip(*(api.tight_box(b["tris"], p, W, H, b["proj"]) for p in b["poses"]))
    return np.stack(t), np.stack(l)


def drawn_count(R):
    """Pixels drawn per render.  Where no fragment lies behind the camera this is count_nonzero; the reference's raster, and the oracle with
    it, gives a fragment behind the camera a NEGATIVE depth, which wins the pixel's minimum over any surface in front and is then no
    surface to anything that reads the image (depth2cloud, score_ref, compose_ref: d > 0).  The box raster must do the same."""
    R = np.asarray(R)
    return np.count_nonzero(R.reshape(len(R), -1) > 0, axis=1)


def class_counts(batches):
    """What the set contains, from the oracle's renders and the host twin only."""
    frame = np.array([0, 0, W - 1, H - 1])
    c = dict(hypotheses=0, frame_loose_own_tight=0, loose_not_frame=0, col_first=0, col_last=0, row_first=0, row_last=0, few_pixels=0, nothing=0,
             one_pixel_boxes=0, behind_camera_fragments=0, offset_decades={})
    for k, b in enumerate(batches):
        tight, loose = batch_boxes(k)
        drawn = b["R"] > 0
        n = drawn.sum((1, 2))
        c["hypotheses"] += len(n)
        whole = (loose == frame).all(1)
        c["frame_loose_own_tight"] += int((whole & (tight != loose).any(1)).sum())
        c["loose_not_frame"] += int((~whole).sum())
        c["col_first"] += int(drawn[:, :, 0].sum()); c["col_last"] += int(drawn[:, :, W - 1].sum())
        c["row_first"] += int(drawn[:, 0, :].sum()); c["row_last"] += int(drawn[:, H - 1, :].sum())
        c["few_pixels"] += int(((n >= 1) & (n <= 25)).sum())
        c["one_pixel_boxes"] += int((n == 1).sum())
        c["nothing"] += int((n == 0).sum())
        c["behind_camera_fragments"] += int((b["R"] < 0).any((1, 2)).sum())
        if b["decade"] is not None:
            c["offset_decades"][b["decade"]] = c["offset_decades"].get(b["decade"], 0) + int((n > 0).sum())
    return c


def assert_classes(batches):
    """What the set must contain for the tests over it to mean anything.  Returns the counts."""
    c = class_counts(batches)
    assert all(len(b["poses"]) <= MAX_BATCH for b in batches)
    assert c["frame_loose_own_tight"] >= 8, c                     # the whole frame as loose box and a tight box of their own
    assert c["loose_not_frame"] >= 8, c
    assert min(c["col_first"], c["col_last"], c["row_first"], c["row_last"]) > 0, c      # drawn pixels in every border column and row
    assert c["few_pixels"] >= 4, c                                # boxes of a few pixels
    assert c["nothing"] >= 2, c
    assert all(c["offset_decades"].get(d, 0) > 0 for d in (3, 4, 5, 6, 7)), c             # every offset decade is present and draws something
    assert 4 * c["nothing"] <= c["hypotheses"], c                 # ... and the set is not mostly empty
    return c


# ---- the pair kernels and the contour fit: references over the same renders ---------------------------------------------------------------
VSD_DELTA = 15.0
FIT_TJR = (0, 10, 0)                                              # the (tau, jump, radius) of test_contour_fit_gpu.TJR at which used, occluded AND miss occur (assert_pair_classes)
FIT_TJR_WIDE = (5, 10, 4)                                         # ... and one with a window, whose nearest edge lies across the box edge (no miss: the noise makes an edge everywhere)
SLACKS = (0, 50)


def vsd_pairing(n):
    """The truth of estimate i is hypothesis perm[i]: the batch rolled by 7, so the shuffled families meet (whole-frame against few-pixel,
    nothing against something, straddle against far)."""
    return np.roll(np.arange(n), 7)


def one_truths(index):
    """(a hypothesis whose box is the frame, one that draws nothing) of batch `index` for the one-truth form: on the mesh batches the
    `close` pose with a whole-frame tight box that draws most and a `nothing` pose, elsewhere the hypotheses that draw most and least."""
    b = stress_batches()[index]
    n = drawn_count(b["R"])
    fam = np.array(b["families"])
    if "close" in b["families"] and "nothing" in b["families"]:
        close = np.flatnonzero((fam == "close") & (batch_boxes(index)[0] == np.array([0, 0, W - 1, H - 1])).all(1))
        return int(close[np.argmax(n[close])]), int(np.flatnonzero(fam == "nothing")[0])
    return int(np.argmax(n)), int(np.argmin(n))


@functools.lru_cache(maxsize=None)
def span_planes(index):
    """(near, far) of batch `index` as the pair kernel reads them (solid_ref.span_ref, raw: INT_MAX / INT_MIN where nothing is drawn)."""
    b = stress_batches()[index]
    return span_ref(b["tris"], b["poses"], b["proj"], W, H, raw=True)


def returned_planes(index):
    """(near, far) as pr_render_span returns them: 0 where nothing is drawn (span_ref with raw=False)."""
    near, far = span_planes(index)
    return np.where(near == INT_MAX, 0, near), np.where(far == INT_MIN, 0, far)


@functools.lru_cache(maxsize=None)
def pair_records(index, slack):
    return pairs_ref(*span_planes(index), slack)


def interleaved(first, second):
    """Two (n, ...) arrays as one (2 n, ...): first[i] at 2 i, second[i] at 2 i + 1."""
    out = np.empty((2 * len(first),) + first.shape[1:], first.dtype)
    out[0::2], out[1::2] = first, second
    return out


def model_centres(index):
    """(centres float32[P, 3] in the camera frame, radius): api._model_center_radius of the batch's mesh, moved by each pose."""
    b = stress_batches()[index]
    cm, rho = api._model_center_radius(api.Model(tris=b["tris"]), None, None)
    return centers(b["poses"], cm), rho


@functools.lru_cache(maxsize=None)
def nearest_map(index, jump, radius):
    return nearest_ref(stress_batches()[index]["scene"], jump, radius)


@functools.lru_cache(maxsize=None)
def fit_reference(index, tjr, roi=NONE):
    """contour_fit_ref.fit_records of batch `index` over the oracle's renders (inside `roi`)."""
    b = stress_batches()[index]
    tau, jump, radius = tjr
    cs, rho = model_centres(index)
    r = b["R"] if roi == NONE else roi_renders(index, roi)
    return fit_records(r, b["scene"], nearest_map(index, jump, radius), tau, jump, b["K"], cs, rho, roi)


@functools.lru_cache(maxsize=None)
def vsd_reference(index, with_k=True):
    b = stress_batches()[index]
    return vsd_ref(b["R"], b["R"][vsd_pairing(len(b["R"]))], b["scene"], b["K"] if with_k else None, VSD_DELTA, SMALL_TAUS)


def pair_class_counts(batches):
    """What the references hold on soup + shell (the two mesh batches): pairs are unordered and off the diagonal."""
    c = dict(both=0, inter=0, zero_rows=0, behind_camera=0, banded=0, small_boxes=0, overlap=0, vsd_inter=0, vsd_far0=0, vsd_zero=0, vsd_one_side=0,
             fit_used=0, fit_occluded=0, fit_miss=0, fit_wide_used=0)
    for k, b in enumerate(batches):
        for rec in fit_reference(k, FIT_TJR):
            c["fit_used"] += rec["used"]; c["fit_occluded"] += rec["occluded"]; c["fit_miss"] += rec["miss"]
        c["fit_wide_used"] += sum(rec["used"] for rec in fit_reference(k, FIT_TJR_WIDE))
        if b["name"] not in ("soup", "shell"):
            continue
        n = len(b["R"])
        upper = np.triu(np.ones((n, n), bool), 1)
        pairs = pair_records(k, 0)
        c["both"] += int(((pairs["both"] > 0) & upper).sum())
        c["inter"] += int(((pairs["inter"] > 0) & upper).sum())
        c["zero_rows"] += int((~pairs.view(np.uint8).reshape(n, -1).any(1)).sum())
        c["behind_camera"] += int((b["R"] < 0).any((1, 2)).sum())
        c["banded"] += sum(area(t) > 8192 for t in batch_boxes(k)[0])           # more than one LDS band in the pair kernel (kSolidTilePx, solid.hip)
        boxes = [box_of_image(r > 0, H) for r in b["R"]]
        c["small_boxes"] += sum(d is not None and 1 <= area(d) <= 25 for d in boxes)
        c["overlap"] += int(((overlap_ref(b["R"], b["scene"], TAU) > 0) & upper).sum())
        v, drawn, perm = vsd_reference(k), drawn_count(b["R"]), vsd_pairing(n)
        c["vsd_inter"] += int((v["inter"] > 0).sum())
        c["vsd_far0"] += int((v["far"][:, 0] > 0).sum())
        c["vsd_zero"] += sum(rec.tobytes() == bytes(rec.nbytes) for rec in v)
        c["vsd_one_side"] += int(((drawn == 0) != (drawn[perm] == 0)).sum())
    return c


def assert_pair_classes(batches):
    """What the set must contain for the tests of the pair kernels and the contour fit to mean anything: floors well below what the
    committed seeds give (profiles/box_stress/README.md).  Returns the counts."""
    c = pair_class_counts(batches)
    assert c["both"] >= 1000 and c["inter"] >= 300, c             # pairs that share pixels, and space
    assert c["zero_rows"] >= 4 and c["behind_camera"] >= 4, c
    assert c["banded"] >= 8 and c["small_boxes"] >= 4, c          # several LDS bands beside boxes of a few pixels
    assert c["overlap"] >= 300, c
    assert c["vsd_inter"] >= 40 and c["vsd_far0"] >= 40 and c["vsd_zero"] >= 8 and c["vsd_one_side"] >= 8, c
    assert min(c["fit_used"], c["fit_occluded"], c["fit_miss"]) > 0 and c["fit_wide_used"] > 0, c
    return c


# ---- the larger sweep of the host test ---------------------------------------------------------------------------------------------------
def sweep_groups(seed=7, scale=1):
    """(name, tris, K, poses) groups of a few thousand poses per family: what the host test walks beyond the committed batches."""
    rng = np.random.default_rng(seed)
    soup, shell = soup_mesh(), shell_mesh()
    K0 = default_K()
    for name, mesh in (("soup", soup), ("shell", shell)):
        yield f"close/{name}", mesh, K0, np.stack([close_pose(rng, mesh, i % 2 == 1) for i in range(1500 * scale)])
        yield f"border/{name}", mesh, K0, np.stack([border_pose(rng, i % 2, 1 - (i & 2)) for i in range(1500 * scale)] + [corner_pose(rng)])
        yield f"far/{name}", mesh, K0, np.stack([far_pose(rng) for _ in range(1500 * scale)])
    for n in range(150 * scale):
        mesh = (soup, shell)[n % 2]
        K = exotic_K(rng)
        yield f"intrinsics/{n}", mesh, K, np.stack([intrinsics_pose(rng, K) for _ in range(20)])
    for n in range(60 * scale):
        o = random_offset(rng, rng.uniform(3.0, 7.5))
        yield f"offset/{n}", offset_mesh((soup, shell)[n % 2], o), K0, np.stack([offset_pose(rng, o) for _ in range(50)])
    for n in range(60 * scale):
        yield f"needle/{n}", needle_mesh(10.0 ** rng.uniform(-3.0, 0.0)), K0, np.stack([random_pose(rng, 300.0) for _ in range(50)])
