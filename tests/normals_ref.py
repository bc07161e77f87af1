"""CPU reference of the normal agreement (pr_score_normals): the definition of include/pose_refine.h in numpy -- differences in int64, the
normals and their comparison in float64 in the header's operand order -- over depth images rendered by the oracle (oracle_lib.render,
bit-exact with the HIP raster), the way verify_ref.py restates pr_score_poses.  It shares no code with the library."""
import numpy as np

from pose_refine_amd import api

FIELDS = ("tested", "agree", "disagree", "no_render_normal", "no_scene_normal")


def _at_offset(d, dx, dy):
    """(value, inside): pixel (x + dx, y + dy) of image d for every (x, y), and whether that pixel lies inside the image."""
    h, w = d.shape
    out, inside = np.zeros_like(d), np.zeros(d.shape, bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = d[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return out, inside


def normal_of(depth, K, step, jump, origin=(0, 0)):
    """The normal of every pixel of the image `depth` (h, w), whose pixel (0, 0) is frame pixel `origin` = (x, y).
    Returns (defined, a, b, c): bool and three float64 arrays; a, b, c mean nothing where `defined` is False."""
    d = np.asarray(depth).astype(np.int64)
    k = np.asarray(K, np.float32).reshape(-1).astype(np.float64)
    fx, cx, fy, cy = k[0], k[2], k[4], k[5]
    hh = int(step)
    (l, in_l), (r, in_r) = _at_offset(d, -hh, 0), _at_offset(d, hh, 0)
    (u, in_u), (dn, in_d) = _at_offset(d, 0, -hh), _at_offset(d, 0, hh)
    defined = d > 0
    for n, inside in ((l, in_l), (r, in_r), (u, in_u), (dn, in_d)):
        defined &= inside & (n > 0) & (np.abs(n - d) <= int(jump))
    gu, gv, z = (r - l).astype(np.float64), (dn - u).astype(np.float64), d.astype(np.float64)
    x = (origin[0] + np.arange(d.shape[1])).astype(np.float64)[None, :]
    y = (origin[1] + np.arange(d.shape[0])).astype(np.float64)[:, None]
    a = -(fx * gu)
    b = -(fy * gv)
    c = (np.float64(2 * hh) * z + (x - cx) * gu) + (y - cy) * gv
    return defined, a, b, c


def agreement(nr, ns, cos_min):
    """Do the normals nr and ns (each (a, b, c)) agree, pixel by pixel?"""
    m = np.float64(np.float32(cos_min))
    with np.errstate(all="ignore"):
        dot = (nr[0] * ns[0] + nr[1] * ns[1]) + nr[2] * ns[2]
        qr = (nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]
        qs = (ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]
        return (dot >= 0) & (dot * dot >= (m * m) * (qr * qs))


def normals_ref(renders, scene, tau, K, step, jump, cos_min, roi=(0, 0, 0, 0)):
    """renders: (P, rh, rw) int32 from oracle_lib.render (0 = nothing drawn; with a ROI, the window's pixels, which are the image of the
    render); scene: (H, W) frame, the scene's image whatever the ROI.  Returns NORMAL[P]."""
    scene = np.asarray(scene)
    sdef, sa, sb, sc = normal_of(scene, K, step, jump)
    x0, y0 = 0, 0
    if roi[2] > 0 and roi[3] > 0:
        x0, y0, w, h = roi
        win = (slice(y0, y0 + h), slice(x0, x0 + w))
        scene, sdef, sa, sb, sc = scene[win], sdef[win], sa[win], sb[win], sc[win]
    s = scene.astype(np.int64)
    out = np.zeros(len(renders), api.NORMAL)
    for i, img in enumerate(np.asarray(renders)):
        r = img.astype(np.int64)
        inlier = (r > 0) & (s > 0) & (np.abs(r - s) <= int(tau))
        if not inlier.any():
            continue
        rdef, ra, rb, rc = normal_of(r, K, step, jump, (x0, y0))
        both = inlier & rdef & sdef
        ok = agreement((ra, rb, rc), (sa, sb, sc), cos_min)
        out[i]["tested"], out[i]["agree"], out[i]["disagree"] = both.sum(), (both & ok).sum(), (both & ~ok).sum()
        out[i]["no_render_normal"], out[i]["no_scene_normal"] = (inlier & ~rdef).sum(), (inlier & rdef & ~sdef).sum()
    return out


def assert_normals_equal(got, want):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:10], got[f][:10], want[f][:10])
    assert got.tobytes() == want.tobytes()                        # (the reserved words are 0 in both)


def assert_identities(normals, scores):
    n = {f: normals[f].astype(np.int64) for f in FIELDS}
    assert np.array_equal(n["tested"], n["agree"] + n["disagree"])
    assert np.array_equal(scores["inlier"].astype(np.int64), n["tested"] + n["no_render_normal"] + n["no_scene_normal"])
    assert (normals["reserved"] == 0).all()
