"""The reference of coarse-to-fine refinement (pr_refine_pyramid), composed from the CPU oracle -- TEST INFRASTRUCTURE.

For one hypothesis: ``O.render`` gives the depth, ``O.depth2cloud(depth, K, 1, tl)`` the stride-1 cloud C1, ``np.nonzero(depth > 0)`` (row-major,
shifted by the ROI origin) the FRAME pixel of every point of C1.  The level cloud of stride s keeps the points with ``x % s == 0 and y % s == 0``;
behind the first level it is moved by the accumulated transform (``po_transform_cloud``, one transform of the original points); ``O.icp`` with the
canonical sums runs on it; ``T_acc = T_l * T_acc`` (``po_mat4_mul``).  The final record is T_acc with the last level's fitness and rmse."""
import ctypes as C

import numpy as np

import oracle_lib as O


def _lib():
    L = O.lib()
    L.po_transform_cloud.restype = None
    L.po_transform_cloud.argtypes = [O.f32p, C.c_size_t, O.f32p]     # exported by liboracle.so, not bound in oracle_lib
    return L


def transform_cloud(cloud, T):
    out = np.array(cloud, dtype=np.float32, order="C", copy=True).reshape(-1, 3)
    if len(out):
        _lib().po_transform_cloud(out.reshape(-1), len(out), np.ascontiguousarray(T, np.float32).reshape(-1))
    return out


def mat4_mul(A, B):
    out = np.zeros(16, np.float32)
    O.lib().po_mat4_mul(np.ascontiguousarray(A, np.float32).reshape(-1), np.ascontiguousarray(B, np.float32).reshape(-1), out)
    return out


def plain_levels(levels):
    """(stride, (relative_fitness, relative_rmse, max_iteration)) tuples from tuples or api.PyramidLevel structures."""
    out = []
    for lv in levels:
        if hasattr(lv, "crit"):
            out.append((int(lv.stride), (float(lv.crit.relative_fitness), float(lv.crit.relative_rmse), int(lv.crit.max_iteration))))
        else:
            out.append((int(lv[0]), (float(lv[1][0]), float(lv[1][1]), int(lv[1][2]))))
    return out


def level_clouds(depth, K, strides, roi=(0, 0, 0, 0)):
    """C1 of one rendered image (the ROI's image when one is given) and, per stride, the boolean mask of the points that level keeps."""
    has_roi = roi[2] > 0 and roi[3] > 0
    tlx, tly = (int(roi[0]), int(roi[1])) if has_roi else (0, 0)
    c1 = O.depth2cloud(depth, K, 1, tlx, tly)
    ys, xs = np.nonzero(depth > 0)                                 # row-major, like depth2cloud's scan
    xs, ys = xs + tlx, ys + tly
    assert len(xs) == len(c1)
    return c1, [(xs % s == 0) & (ys % s == 0) for s in strides]


def refine_pyramid(tris, poses, width, height, proj, K, scene, levels, ppb, roi=(0, 0, 0, 0)):
    """(records[P], level_records[L, P], level_sizes[L, P]) of the composition above, ``scene`` an oracle_lib scene."""
    levels = plain_levels(levels)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    P, L = len(poses), len(levels)
    res = np.zeros(P, O.RESULT)
    lres = np.zeros((L, P), O.RESULT)
    lsizes = np.zeros((L, P), np.uint32)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    for i in range(P):
        depth = O.render(tris, poses[i:i + 1], width, height, proj, roi)[0]
        c1, keep = level_clouds(depth, K, [s for s, _ in levels], roi)
        t_acc = eye.copy()
        for l, (s, crit) in enumerate(levels):
            cloud = np.ascontiguousarray(c1[keep[l]])
            if l > 0:
                cloud = transform_cloud(cloud, t_acc)
            rec = np.zeros(1, O.RESULT)[0]
            rec["T"] = eye
            if len(cloud):
                rec = O.icp(cloud, scene, crit, O.SUM_CANONICAL, ppb)[0]
            lres[l, i] = rec
            lsizes[l, i] = len(cloud)
            t_acc = mat4_mul(rec["T"], t_acc)
        res[i]["T"] = t_acc
        res[i]["fitness"] = lres[L - 1, i]["fitness"]
        res[i]["inlier_rmse"] = lres[L - 1, i]["inlier_rmse"]
    return res, lres, lsizes
