"""CPU reference of pr_score_overlap and pr_select_greedy: the inlier masks exactly as verify_ref.score_ref forms them over the oracle's renders
(oracle_lib.render), their pairwise intersections counted in integers, and the greedy rule in Python integers.  Also the planted frame the
selection tests share."""
import numpy as np

from pose_refine_amd import synth

BLOCK = 1 << 16         # pixels per product below: a float32 sum of at most 65536 ones is exact


def support_ref(render, scene, tau):
    """(rh, rw) bool: the pixels score_ref counts as `inlier` for one render (scene already cut to the ROI window)."""
    r = np.asarray(render).astype(np.int64)
    s = np.asarray(scene).astype(np.int64)
    return (r > 0) & (s > 0) & (np.abs(r - s) <= tau)


def overlap_of_supports(supports):
    """supports: per hypothesis the sorted flat indices of its inlier pixels.  mask @ mask.T in int64, formed over the pixels that occur at
    all, BLOCK of them at a time (each block's product is exact in float32 and is added up in int64)."""
    P = len(supports)
    out = np.zeros((P, P), np.int64)
    if P == 0:
        return out
    union = np.unique(np.concatenate([np.asarray(s, np.int64) for s in supports]))
    pos = [np.searchsorted(union, s) for s in supports]
    for b0 in range(0, len(union), BLOCK):
        b1 = min(b0 + BLOCK, len(union))
        m = np.zeros((P, b1 - b0), np.float32)
        for i, p in enumerate(pos):
            lo, hi = np.searchsorted(p, (b0, b1))
            m[i, p[lo:hi] - b0] = 1.0
        out += np.rint(m @ m.T).astype(np.int64)
    return out


def overlap_ref(renders, scene, tau, roi=(0, 0, 0, 0)):
    """renders: (P, rh, rw) int32 from oracle_lib.render, or any iterable of (rh, rw) renders (one at a time: large frames);
    scene: (H, W) frame.  Returns int64[P, P]: the number of pixels that are inliers of both i and j."""
    scene = np.asarray(scene)
    if roi[2] > 0 and roi[3] > 0:
        x, y, w, h = roi
        scene = scene[y:y + h, x:x + w]
    return overlap_of_supports([np.flatnonzero(support_ref(r, scene, tau)) for r in renders])


def greedy_ref(order, overlap, shared_num, shared_den):
    """pr_select_greedy's rule in Python integers."""
    ov = np.asarray(overlap)
    sel = []
    for i in (int(v) for v in order):
        own = int(ov[i, i])
        if own == 0:
            continue
        if all(int(ov[i, j]) * int(shared_den) <= int(shared_num) * min(own, int(ov[j, j])) for j in sel):
            sel.append(i)
    return sel


def rank_fraction(scores):
    sc = np.asarray(scores)
    den = sc["visible"].astype(np.int64) - sc["occluded"].astype(np.int64)
    return np.where(den <= 0, 0.0, sc["inlier"].astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))


# ---- the planted frame: three instances of one object, 85 hypotheses around each ------------------------------------------------------
PLANTED_SHIFTS = ((-70, 0, 60), (0, 0, 0), (150, 40, 0))
PLANTED_EXACT = [0, 85, 170]            # instance k's exact pose
PLANTED_SELECTION = [170, 85, 0]


def shift(dx, dy, dz):
    m = np.zeros((4, 4), np.float32)
    m[:3, 3] = (dx, dy, dz)
    return m


def planted_frame(render, tris, W, H, proj):
    """(scene int32 (H, W), poses float32 (255, 4, 4)).  render: oracle_lib.render."""
    S = synth.scene_pose()
    inst = [S + shift(*d) for d in PLANTED_SHIFTS]
    r = render(tris, np.stack(inst), W, H, proj).astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    rng = np.random.default_rng(20)
    scene = scene + np.where(rng.random(scene.shape) < 0.4, rng.integers(-3, 4, scene.shape), 0) * (scene > 0)
    bg = scene == 0
    scene[bg & (rng.random(scene.shape) < 0.5)] = 900
    scene[rng.random(scene.shape) < 0.08] = 0
    hy = synth.hypotheses(256)
    poses = [inst[k] if j < 0 else hy[1 + 84 * k + j] + shift(*PLANTED_SHIFTS[k]) for k in range(3) for j in range(-1, 84)]
    return scene.astype(np.int32), np.stack(poses).astype(np.float32)
