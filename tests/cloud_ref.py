"""Scenes from point clouds: a numpy restatement of include/pose_refine.h's definition of the k nearest neighbours of a scene point and of its PCA
normal, and the clouds test_cloud_host.py and test_cloud_gpu.py share.  It shares no code with the library: the neighbours are brute force over all
pairs in float32, in the stated expression order, with a stable sort on (d2, j); the normal is IEEE double arithmetic in list order (the sums as
numpy float64 columns, one neighbour after the other; the Jacobi in Python floats, written out), every product formed and then added."""
import functools
import math

import numpy as np

KNN_NONE = 0xFFFFFFFF
MAX_SWEEPS = 16                                       # PR_PLANE_MAX_SWEEPS


class Brute:
    """All pairs of one cloud (in the order given): d2[i, j] and, per i, the candidates j in ascending (d2, j)."""

    def __init__(self, points):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.points = p
        d = p[None, :, :] - p[:, None, :]                                                   # d[i, j] = p_j - p_i, float32
        self.d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        self.order = np.argsort(self.d2, axis=1, kind="stable")                            # stable: a tie in d2 keeps the lower j first

    def knn(self, k, max_radius):
        """(idx uint32[n, k], d2 float32[n, k], count uint32[n])."""
        n = len(self.points)
        r2 = np.float32(max_radius) * np.float32(max_radius)
        kk = min(k, n)
        first = self.order[:, :kk]
        dist = np.take_along_axis(self.d2, first, axis=1)
        ok = dist <= r2                                                                     # sorted: the admissible ones are a prefix
        idx = np.full((n, k), KNN_NONE, np.uint32)
        d2 = np.zeros((n, k), np.float32)
        idx[:, :kk] = np.where(ok, first, KNN_NONE)
        d2[:, :kk] = np.where(ok, dist, np.float32(0))
        return idx, d2, ok.sum(axis=1).astype(np.uint32)


def jacobi3(a, max_sweeps=MAX_SWEEPS):
    """The cyclic Jacobi of pose_refine.h on a symmetric 3 x 3 (lists of Python floats): (diagonal, V) with V's columns the eigenvectors."""
    A = [list(r) for r in a]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(max_sweeps):
        off = max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2]))
        diag = max(abs(A[0][0]), abs(A[1][1]), abs(A[2][2]))
        if off <= 2.0 ** -56 * diag:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] -= t * apq
            A[q][q] += t * apq
            A[p][q] = 0.0
            A[q][p] = 0.0
            k = 3 - p - q
            akp, akq = A[k][p], A[k][q]
            np_, nq = c * akp - s * akq, s * akp + c * akq
            A[k][p] = np_; A[p][k] = np_
            A[k][q] = nq; A[q][k] = nq
            for r in range(3):
                vp, vq = V[r][p], V[r][q]
                V[r][p] = c * vp - s * vq
                V[r][q] = s * vp + c * vq
    return [A[0][0], A[1][1], A[2][2]], V


def scatter(points, idx, count):
    """Centroid and the six scatter sums of every point's list, in list order, float64: (c[n, 3], S[n, 6]) with S = xx, xy, xz, yy, yz, zz."""
    p = np.asarray(points, np.float32).astype(np.float64)
    n, k = idx.shape
    c = np.zeros((n, 3))
    for t in range(k):
        use = t < count
        c[use] = c[use] + p[idx[use, t]]
    c = c / np.maximum(count, 1)[:, None].astype(np.float64)
    S = np.zeros((n, 6))
    for t in range(k):
        use = t < count
        d = p[idx[use, t]] - c[use]
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1)
        S[use] = S[use] + prod
    return c, S


def normals(points, idx, count, min_neighbours=3, line_ratio=1e-4, viewpoint=(0.0, 0.0, 0.0)):
    """(normal float32[n, 3], variation float32[n], counts dict) from the lists."""
    p32 = np.asarray(points, np.float32)
    n = len(p32)
    _, S = scatter(p32, idx, count)
    out = np.zeros((n, 3), np.float32)
    var = np.zeros(n, np.float32)
    counts = dict(points=n, with_normal=0, too_few=0, degenerate=0)
    lr = float(np.float32(line_ratio))
    vp = [float(np.float32(v)) for v in viewpoint]
    for i in range(n):
        if count[i] < min_neighbours:
            counts["too_few"] += 1
            continue
        xx, xy, xz, yy, yz, zz = (float(v) for v in S[i])
        lam, V = jacobi3([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        lo = min(range(3), key=lambda a: (lam[a], a))
        rest = [a for a in range(3) if a != lo]
        mid = min(rest, key=lambda a: (lam[a], a))
        hi = rest[0] if rest[1] == mid else rest[1]
        if lam[mid] <= lr * lam[hi]:
            counts["degenerate"] += 1
            continue
        nx, ny, nz = V[0][lo], V[1][lo], V[2][lo]
        vx, vy, vz = vp[0] - float(p32[i, 0]), vp[1] - float(p32[i, 1]), vp[2] - float(p32[i, 2])
        if (nx * vx + ny * vy) + nz * vz < 0.0:
            nx, ny, nz = -nx, -ny, -nz
        out[i] = (np.float32(nx), np.float32(ny), np.float32(nz))
        var[i] = np.float32(lam[lo] / ((lam[lo] + lam[mid]) + lam[hi]))
        counts["with_normal"] += 1
    return out, var, counts


def angle(a, b, signed=False):
    """Angle in radians between the rows of a and b (float64; atan2 of |a x b| and a . b, exact near 0), up to sign unless `signed`."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cr = np.linalg.norm(np.cross(a, b), axis=-1)
    dt = (a * b).sum(-1)
    return np.arctan2(cr, dt if signed else np.abs(dt))


# ---- the clouds ---------------------------------------------------------------------------------------------------------------------------------
def random_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def lattice():
    """A 9 x 9 x 3 integer lattice scaled by 2^-6: every distance is exact, the ties are exact ties and only the index rule decides."""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g.astype(np.float32) * np.float32(2.0 ** -6))


def two_clusters():
    """Two clusters of six points a metre apart: within max_radius = 0.2 a point has six candidates, fewer than k = 8."""
    rng = np.random.default_rng(11)
    a = rng.random((6, 3)).astype(np.float32) * np.float32(0.05)
    return np.concatenate([a, a[::-1] * np.float32(0.9) + np.float32(1.0)]).astype(np.float32)


def tilted_planes(n_per=400, seed=5):
    """float32 points placed analytically on three planes (one frontal, two tilted, half a metre apart) in front of a camera at the origin: (points, true unit normals float64)."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for normal, origin in (((0.0, 0.0, -1.0), (0.0, 0.0, 0.8)), ((0.3, -0.2, -1.0), (0.5, 0.0, 0.6)), ((-0.6, 0.5, -0.4), (-0.5, 0.1, 0.9))):
        nv = np.array(normal) / np.linalg.norm(normal)
        u = np.cross(nv, (0.0, 1.0, 0.0)); u /= np.linalg.norm(u)
        v = np.cross(nv, u)
        ab = rng.uniform(-0.15, 0.15, size=(n_per, 2))
        pts.append((np.array(origin) + ab[:, :1] * u + ab[:, 1:] * v).astype(np.float32))
        nrm.append(np.repeat(nv[None], n_per, 0))
    return np.concatenate(pts), np.concatenate(nrm)


SPHERE_CENTRE, SPHERE_RADIUS = np.array([0.05, -0.02, 0.7]), 0.12


def sphere(n=1500, seed=9):
    """float32 points placed analytically on a sphere: (points, true outward unit normals float64)."""
    g = np.random.default_rng(seed).normal(size=(n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return (SPHERE_CENTRE + SPHERE_RADIUS * g).astype(np.float32), g


@functools.lru_cache(maxsize=None)
def cases():
    """Every (name, points, max_leaf, k, max_radius) both test files run; `generic`: False for the lattice alone, whose neighbourhoods are
    symmetric by construction -- exactly repeated eigenvalues, no defined eigenvector to compare with."""
    out = []
    add = lambda name, pts, max_leaf, k, r=math.inf, generic=True: out.append(dict(name=name, points=pts, max_leaf=max_leaf, k=k, max_radius=r, generic=generic))
    for n in (1, 2, 3):
        add(f"n{n}_k8", random_cloud(n, 100 + n), 10, 8)                                   # k > n
    for n in (63, 64, 65, 257):
        add(f"n{n}", random_cloud(n, n), 10, 8)                                            # lane and workgroup edges
    add("identical", np.repeat(np.array([[0.25, -0.5, 0.75]], np.float32), 40, 0), 4, 8)
    add("lattice", lattice(), 4, 10, generic=False)
    add("clusters", two_clusters(), 3, 8, 0.2)
    big = random_cloud(2000, 2000)
    for max_leaf in (1, 10):
        for k in (1, 3, 8, 16, 32):
            for r in (math.inf, 0.12):
                add(f"random2000_leaf{max_leaf}_k{k}_r{r}", big, max_leaf, k, r)
    add("planes", tilted_planes()[0], 10, 16)
    add("sphere", sphere()[0], 10, 16)
    return tuple(out)
