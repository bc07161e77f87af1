"""A bit-exact Python restatement of the per-iteration update (pose_refine_amd/csrc/pr_solver.inl and the iteration logic of
icp.cu:178-212 as pr_icp.cpp's pose_iteration_host runs it), and a corpus of 29-sum systems built from fixed seeds.

Python floats are IEEE binary64 with one rounding per operation, which is what the C++ computes with contraction off; every
double -> float cast goes through np.float32 (round to nearest even).  Float32 arithmetic (the 4x4 product, the scores) is done
in double and rounded once per operation: for +, -, *, / and sqrt that is the correctly rounded float32 result, since
53 >= 2 * 24 + 2.  The restatement follows the C++ operation by operation, including the adds of 0.0 and the products with 0.0
that decide signed zeros and NaN propagation.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

TINY = 1.0 / 1.7976931348623157e308
QUARTER_PI = 0.78539816339744830962
TWO_OVER_PI = 0.63661977236758134308
PIO2 = (float.fromhex("0x1.921fb0p+0"), float.fromhex("0x1.5110b0p-22"), float.fromhex("0x1.184698p-44"),
        float.fromhex("0x1.3198a2e037073p-69"))


def f32(v: float) -> float:
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(v))


def dabs(v: float) -> float:
    return -v if v < 0 else v


# ---- sin / cos (prs::ksin, prs::kcos, prs::sincos_d) -----------------------------------------------------------------------
def ksin(x: float) -> float:
    z = x * x
    p = 1.58969099521155010221e-10
    p = p * z + -2.50507602534068634195e-08
    p = p * z + 2.75573137070700676789e-06
    p = p * z + -1.98412698298579493134e-04
    p = p * z + 8.33333333332248946124e-03
    p = p * z + -1.66666666666666324348e-01
    return x + (x * z) * p


def kcos(x: float) -> float:
    z = x * x
    p = -1.13596475577881948265e-11
    p = p * z + 2.08757232129817482790e-09
    p = p * z + -2.75573143513906633035e-07
    p = p * z + 2.48015872894767294178e-05
    p = p * z + -1.38888888888741095749e-03
    p = p * z + 4.16666666666666019037e-02
    return (1.0 - 0.5 * z) + (z * z) * p


def sincos_branch(x: float) -> str:
    if dabs(x) <= QUARTER_PI:
        return "kernel"
    if not dabs(x) < 1.0e9:
        return "cut"
    return "reduced"


def sincos_d(x: float):
    if dabs(x) <= QUARTER_PI:
        return ksin(x), kcos(x)
    if not dabs(x) < 1.0e9:
        return 0.0, 1.0
    t = x * TWO_OVER_PI
    n = int(t - 0.5 if t < 0 else t + 0.5)              # C cast: truncation toward zero
    fn = float(n)
    r = (((x - fn * PIO2[0]) - fn * PIO2[1]) - fn * PIO2[2]) - fn * PIO2[3]
    sr, cr = ksin(r), kcos(r)
    q = n & 3                                           # two's complement, as (int)(n & 3) on a long long
    if q == 0:
        return sr, cr
    if q == 1:
        return cr, -sr
    if q == 2:
        return -sr, -cr
    return -cr, sr


# ---- prs::ldlt6 -------------------------------------------------------------------------------------------------------------
@dataclass
class SolveInfo:
    pivots: tuple = ()          # s0..s5 (s5 is always 5)
    dk_zero: int = 0            # steps whose dk was 0 (or NaN): the column below is left undivided
    tiny: int = 0               # diagonal entries at or below 1/DBL_MAX in magnitude: the pseudo-inverse gives 0
    ties: int = 0               # pivot candidates equal in magnitude to the running maximum (the strict > keeps the earlier row)
    sincos: tuple = ()          # branch of sincos_d for each half-angle
    half_angles: tuple = ()


def _sym_swap(m, K, P):
    for j in range(K):
        m[K][j], m[P][j] = m[P][j], m[K][j]
    for i in range(P + 1, 6):
        m[i][K], m[i][P] = m[i][P], m[i][K]
    for i in range(K + 1, P):
        m[i][K], m[P][i] = m[P][i], m[i][K]
    m[K][K], m[P][P] = m[P][P], m[K][K]


def _ldlt6_step(m, K, info: SolveInfo) -> int:
    p = K
    top = dabs(m[K][K])
    for i in range(K + 1, 6):
        a = dabs(m[i][i])
        if a == top:
            info.ties += 1
        if a > top:
            top = a
            p = i
    if p != K:
        _sym_swap(m, K, p)
    w = [0.0] * 6
    dot = 0.0
    for j in range(K):
        w[j] = m[j][j] * m[K][j]
        dot += m[K][j] * w[j]
    m[K][K] -= dot
    dk = m[K][K]
    if not dabs(dk) > 0.0:
        info.dk_zero += 1
    for i in range(K + 1, 6):
        acc = 0.0
        for j in range(K):
            acc += m[i][j] * w[j]
        v = m[i][K] - acc
        m[i][K] = v / dk if dabs(dk) > 0.0 else v
    return p


def _perm_apply(y, K, p):
    if p != K:
        y[K], y[p] = y[p], y[K]


def ldlt6(m, rhs, info: SolveInfo):
    s = [_ldlt6_step(m, K, info) for K in range(6)]
    info.pivots = tuple(s)
    y = list(rhs)
    for K in range(5):
        _perm_apply(y, K, s[K])
    for i in range(1, 6):
        for j in range(i):
            y[i] -= m[i][j] * y[j]
    for i in range(6):
        if dabs(m[i][i]) > TINY:
            y[i] = y[i] / m[i][i]
        else:
            info.tiny += 1
            y[i] = 0.0
    for i in range(4, -1, -1):
        for j in range(i + 1, 6):
            y[i] -= m[j][i] * y[j]
    for K in range(4, -1, -1):
        _perm_apply(y, K, s[K])
    return y


def compose_update(u, sx, cx, sy, cy, sz, cz):
    aw = cz * cy - 0.0 * 0.0 - 0.0 * sy - sz * 0.0
    ax = cz * 0.0 + 0.0 * cy + 0.0 * 0.0 - sz * sy
    ay = cz * sy + 0.0 * cy + sz * 0.0 - 0.0 * 0.0
    az = cz * 0.0 + sz * cy + 0.0 * sy - 0.0 * 0.0
    qw = aw * cx - ax * sx - ay * 0.0 - az * 0.0
    qx = aw * sx + ax * cx + ay * 0.0 - az * 0.0
    qy = aw * 0.0 + ay * cx + az * sx - ax * 0.0
    qz = aw * 0.0 + az * cx + ax * 0.0 - ay * sx
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    T = [1.0 - (tyy + tzz), txy - twz, txz + twy, u[3],
         txy + twz, 1.0 - (txx + tzz), tyz - twx, u[4],
         txz - twy, tyz + twx, 1.0 - (txx + tyy), u[5],
         0.0, 0.0, 0.0, 1.0]
    return np.array([f32(v) for v in T], np.float32)


def solve_666(A36, b6):
    """prs::solve_666_impl: A (36 floats, symmetric, any major), b (6 floats) -> (T as 16 float32, SolveInfo)."""
    A = [float(v) for v in np.asarray(A36, np.float32).reshape(36)]
    b = [float(v) for v in np.asarray(b6, np.float32).reshape(6)]
    m = [[A[c * 6 + r] + (0.01 if r == c else 0.0) for c in range(6)] for r in range(6)]
    info = SolveInfo()
    u = ldlt6(m, b, info)
    half = (0.5 * u[0], 0.5 * u[1], 0.5 * u[2])
    sx, cx = sincos_d(half[0])
    sy, cy = sincos_d(half[1])
    sz, cz = sincos_d(half[2])
    info.sincos = tuple(sincos_branch(h) for h in half)
    info.half_angles = half
    return compose_update(u, sx, cx, sy, cy, sz, cz), info


def mat4_mul(A, B):
    """prs::mat4_mul_impl: C = A * B in float32, each entry summed over index 3, 2, 1, 0 starting from 0."""
    A = [float(v) for v in np.asarray(A, np.float32).reshape(16)]
    B = [float(v) for v in np.asarray(B, np.float32).reshape(16)]
    C = np.zeros(16, np.float32)
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in (3, 2, 1, 0):
                acc = f32(acc + f32(A[i * 4 + k] * B[k * 4 + j]))
            C[i * 4 + j] = acc
    return C


def sums_to_A(sums):
    """The 21 upper-triangle sums row by row -> the symmetric 36 (icp.cu:196-205)."""
    A = np.zeros(36, np.float32)
    k = 0
    for y in range(6):
        for x in range(y, 6):
            A[x + y * 6] = sums[k]
            A[y + x * 6] = sums[k]
            k += 1
    return A


def A_to_sums(A):
    A = np.asarray(A, np.float32).reshape(6, 6)
    return np.array([A[y, x] for y in range(6) for x in range(y, 6)], np.float32)


def pose_iteration(sums, n_points, T, rmse, fitness, crit, it):
    """One iteration of pose_iteration_host / pose_iteration_wave.  crit: (relative_fitness, relative_rmse, max_iteration).
    Returns (T, rmse, fitness, E or None (finished), SolveInfo or None)."""
    s = np.asarray(sums, np.float32)
    cnt, err = float(s[28]), float(s[27])
    if cnt == 0:
        return np.asarray(T, np.float32).reshape(16).copy(), rmse, fitness, None, None
    prev_fit, prev_rmse = f32(fitness), f32(rmse)
    fitness = f32(cnt / f32(float(n_points)))
    q = f32(err / cnt)
    rmse = f32(math.sqrt(q)) if q >= 0 else (q if q != q else math.nan)
    T = np.asarray(T, np.float32).reshape(16).copy()
    if it == int(np.uint32(np.int32(crit[2]))):
        return T, rmse, fitness, None, None
    rf, rr = f32(crit[0]), f32(crit[1])
    df, dr = f32(fitness - prev_fit), f32(rmse - prev_rmse)
    if dabs(df) < rf and dabs(dr) < rr:
        return T, rmse, fitness, None, None
    E, info = solve_666(sums_to_A(s[:21]), s[21:27])
    return mat4_mul(E, T), rmse, fitness, E, info


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
@dataclass
class Batch:
    """Systems that go through one pr_debug_pose_iteration call (one criteria / iteration for the batch)."""
    name: str
    sums: np.ndarray                    # (n, 29) float32
    n_points: np.ndarray                # (n,) uint32
    crit: tuple = (0.0, 0.0, 100)       # relative_fitness 0: never converged -> the solve always runs when cnt != 0 and it != max
    it: int = 0
    T: np.ndarray = None                # (n, 16) prior transforms (default identity)
    rmse: np.ndarray = None
    fitness: np.ndarray = None
    tags: list = field(default_factory=list)

    def __post_init__(self):
        n = len(self.sums)
        if self.T is None:
            self.T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))
        if self.rmse is None:
            self.rmse = np.zeros(n, np.float32)
        if self.fitness is None:
            self.fitness = np.zeros(n, np.float32)
        if not self.tags:
            self.tags = [self.name] * n


def system(A, b, cnt=100.0, err=1.0):
    s = np.zeros(29, np.float32)
    s[:21] = A_to_sums(A)
    with np.errstate(over="ignore"):
        s[21:27] = np.asarray(b, np.float32)
    s[27] = err
    s[28] = cnt
    return s


def ALL_PIVOT_SEQUENCES():
    import itertools
    return [tuple(v) + (5,) for v in itertools.product(*[range(K, 6) for K in range(5)])]


def _order_for(seq):
    """The original indices in the order the pivoting visits them when it takes pivot rows seq: rank r = the r-th pivot."""
    cur = list(range(6))
    for K in range(5):
        p = seq[K]
        cur[K], cur[p] = cur[p], cur[K]
    return cur


def pivot_systems(seed=1234, spd_per_seq=3):
    """All 720 pivot sequences: (a) a diagonal in the target order plus small symmetric noise; (b) random SPD systems L D L^T with
    log-uniform scales whose pivot order is the target (drawn until the restatement confirms it).  Returns (sums list, tags)."""
    rng = np.random.default_rng(seed)
    out, tags = [], []
    for seq in ALL_PIVOT_SEQUENCES():
        order = _order_for(seq)
        d = np.zeros(6)
        for rank, orig in enumerate(order):
            d[orig] = 2.0 ** (12 - 3 * rank) * (1.0 + 0.5 * rng.random())
        noise = rng.normal(size=(6, 6)) * 1e-3
        noise = (noise + noise.T) * np.sqrt(np.outer(d, d))
        A = np.diag(d) + noise * (1 - np.eye(6))
        out.append(system(A, rng.normal(size=6))); tags.append("pivot-diag")
        got = 0
        for _ in range(60):
            if got == spd_per_seq:
                break
            gaps = rng.uniform(1.0, 2.2, 5)                              # decades between consecutive pivots, all within 1e-6 .. 1e6
            top = rng.uniform(-6.0 + gaps.sum(), 6.0)
            Dv = 10.0 ** (top - np.concatenate([[0.0], np.cumsum(gaps)]))
            L = np.eye(6) + np.tril(rng.uniform(-0.3, 0.3, (6, 6)) * np.sqrt(np.outer(Dv, 1.0 / Dv)), -1)   # correlations below 0.3
            B = (L * Dv) @ L.T
            A = np.empty((6, 6))
            A[np.ix_(order, order)] = B
            A = np.asarray((A + A.T) / 2, np.float32)
            s = system(A, rng.normal(size=6) * np.sqrt(np.diag(A).astype(np.float64) + 1e-3))
            if solve_666(sums_to_A(s[:21]), s[21:27])[1].pivots == seq:
                out.append(s); tags.append("pivot-spd"); got += 1
    return out, tags


def edge_systems(seed=99):
    """Branch edges of the solve.  Returns (sums list, tags)."""
    rng = np.random.default_rng(seed)
    out, tags = [], []

    def add(tag, A, b, **kw):
        out.append(system(A, b, **kw)); tags.append(tag)
    b = rng.normal(size=6)
    add("tie", np.eye(6) * 3.0, b)                                       # all six equal: the first row wins every step
    add("tie", np.diag([2.0, 5.0, 5.0, 1.0, 5.0, 2.0]), b)
    add("tie-sign", np.diag([4.0, -4.0, 4.0, -4.0, 1.0, 1.0]), b)       # equal magnitudes, opposite signs
    add("tie-sign", np.diag([-0.5, 0.5, -7.0, 7.0, -7.0, 0.25]), b)
    t = np.diag([6.0, 2.0, 3.0, 4.0, 5.0, 6.0]); t[5, 0] = t[0, 5] = 0.5                # a tie at step 0 between coupled rows
    add("tie", t, b)
    # ties whose rows couple differently to the rest: taking the later row instead of the earlier one changes the rounding
    for k in range(24):
        M = rng.normal(size=(6, 6)); S = M @ M.T * 0.05
        mags = np.repeat(rng.uniform(1.0, 100.0, 3), 2)
        perm = rng.permutation(6)
        d = mags[perm] * (rng.choice([-1.0, 1.0], 6) if k % 2 else 1.0)
        np.fill_diagonal(S, d)
        add("tie-coupled", np.asarray(S, np.float32), rng.normal(size=6))
    # a tie inside a singular 2x2 block [[h, h], [h, h]] (h = 2^60 hides the 0.01): the row taken first keeps its D, the other one's
    # dk is exactly 0 and its D is pseudo-inverted to 0 -- which row that is decides the solution, not just its rounding
    for k in range(12):
        i, j = sorted(rng.choice(6, 2, replace=False))
        S = np.diag(rng.uniform(1.0, 100.0, 6))
        c = rng.uniform(-1.0, 1.0, (6, 6)); c = (c + c.T) / 2
        S += c * (1 - np.eye(6))
        h = 2.0 ** 60
        S[i, i] = S[j, j] = S[i, j] = S[j, i] = h
        add("tie-singular", np.asarray(S, np.float32), rng.normal(size=6))
    add("zero", np.zeros((6, 6)), b)
    add("zero", np.zeros((6, 6)), np.zeros(6))
    for rank in range(1, 6):                                             # planar / cylindrical geometry: J J^T of rank < 6
        J = rng.normal(size=(rank, 6)) * np.array([1, 1, 1, 0.2, 0.2, 0.2])
        for scale in (1.0, 1e4):
            A = np.asarray(J.T @ J * scale, np.float32)
            add(f"rank{rank}", A, J.T @ rng.normal(size=rank) * scale)
    for _ in range(4):
        M = rng.normal(size=(6, 6)); A = (M + M.T) * 3
        add("indefinite", A, rng.normal(size=6))
    add("dk-small", np.diag([-0.01, 1.0, 2.0, 3.0, 4.0, 5.0]), b)        # float(-0.01f) + 0.01 = 2.2e-10 in double: tiny, not 0
    c = np.diag([2.0 ** 60, 2.0 ** 60, 1.0, 2.0, 3.0, 4.0]); c[0, 1] = c[1, 0] = 2.0 ** 60
    c[2:, 0] = c[0, 2:] = [0.5, 0.25, 1.0, 2.0]                          # 0.01 vanishes next to 2^60: the second pivot's dk is exactly 0
    add("dk0", c, b)
    c = np.diag([1.0, 2.0, 3.0, 4.0, 2.0 ** 70, 2.0 ** 70]); c[4, 5] = c[5, 4] = -(2.0 ** 70)
    c[:4, 5] = c[5, :4] = [1.0, -1.0, 0.5, 3.0]
    add("dk0", c, b)
    add("b0", np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) + 0.1, np.zeros(6))
    M = rng.normal(size=(6, 6)); S = M @ M.T
    add("huge", S / np.abs(S).max() * 1e30, rng.normal(size=6) * 1e30)
    add("huge", np.eye(6) * 3e38, rng.normal(size=6) * 3e38)
    add("denormal", np.eye(6) * 1e-40, np.full(6, 1e-40))
    add("denormal", S * 1e-40, rng.normal(size=6) * 1e-40)
    D = np.diag([1e-40, 2.0, 1e-41, 3.0, 5e-42, 1.0]); D[0, 1] = D[1, 0] = 1e-40
    add("denormal", D, np.array([1e-40, 1.0, -1e-40, 1.0, 1e-45, 2.0]))
    return out, tags


def angle_systems():
    """Half-angles chosen through b: with A = 2^53 I, m = 2^53 exactly (0.01 is below half an ulp) and u = b / 2^53 exactly, so a
    float32 b = x * 2^54 gives the half-angle x.  Returns (sums list, tags)."""
    P = float(2 ** 53)
    below = float(np.nextafter(np.float32(QUARTER_PI), np.float32(0)))
    above = float(np.nextafter(np.float32(QUARTER_PI), np.float32(1)))
    near = float(np.float32(QUARTER_PI))
    halves = [0.0, -0.0, below, near, above, -above, float(np.float32(math.pi / 2)), float(np.float32(math.pi)), -float(np.float32(math.pi)),
              1e3, -1e3, 1e5, 12345.678, 3.0e7, float(np.nextafter(np.float32(1e9), np.float32(0))), 1e9, -1e9, 4e9, math.nan]
    out, tags = [], []
    for h in halves:
        b = np.array([h * 2.0 ** 54, 0.25 * 2.0 ** 54, -h * 2.0 ** 54 if h == h else 1.0, 1.0, 2.0, 3.0])
        A = np.eye(6) * P
        out.append(system(A, b)); tags.append("angle")
    return out, tags


def nonfinite_systems(seed=7):
    rng = np.random.default_rng(seed)
    out, tags = [], []
    M = rng.normal(size=(6, 6)); S = M @ M.T + np.eye(6)
    for k, v in ((0, math.nan), (3, math.inf), (10, -math.inf), (20, math.nan)):
        s = system(S, rng.normal(size=6)); s[k] = v
        out.append(s); tags.append("nonfinite-A")
    for k, v in ((21, math.nan), (24, math.inf), (26, -math.inf)):
        s = system(S, rng.normal(size=6)); s[k] = v
        out.append(s); tags.append("nonfinite-b")
    return out, tags


def icp_systems(scenario, n_proj=16, n_nn=2, passes=20):
    """The oracle's canonical 29-sum traces of configs[1] (projective) hypotheses and of configs[2] (kd-tree) ones."""
    import oracle_lib as O
    from pose_refine_amd import synth
    ppb = 2048
    out, tags = [], []
    poses = synth.hypotheses(256)
    for kind, picks in (("proj", range(0, 256, 256 // n_proj)), ("nn", range(0, 256, 256 // n_nn))):
        scene = scenario["proj_scene" if kind == "proj" else "nn_scene"]
        for i in picks:
            depth = O.render(scenario["tris"], poses[i:i + 1], synth.WIDTH, synth.HEIGHT, scenario["proj"])[0]
            cloud = O.depth2cloud(depth, scenario["K"])
            if len(cloud) == 0:
                continue
            _, _, _, tr = O.icp(cloud, scene, (0.0, 0.0, passes if kind == "proj" else 4), O.SUM_CANONICAL, ppb, trace=True)
            for row in tr:
                if row[28] != 0:
                    out.append(np.asarray(row, np.float32)); tags.append("icp-" + kind)
    return out, tags


def solve_batches(scenario=None):
    """Every solve-corpus system as one batch (identity prior, never converged, iteration 0, count 100 of 1000 points) plus a copy
    of the pivot family with a non-identity prior T."""
    parts = [pivot_systems(), edge_systems(), angle_systems(), nonfinite_systems()]
    if scenario is not None:
        parts.append(icp_systems(scenario))
    sums = [s for p in parts for s in p[0]]
    tags = [t for p in parts for t in p[1]]
    sums = np.asarray(sums, np.float32)
    n_pts = np.where(sums[:, 28] > 0, np.maximum(sums[:, 28], 1.0), 1000.0).astype(np.uint32)
    batches = [Batch("solve", sums, n_pts, tags=tags)]
    rng = np.random.default_rng(5)
    k = min(len(sums), 400)
    T = np.zeros((k, 16), np.float32)
    for i in range(k):
        E, _ = solve_666(sums_to_A(np.array([0.0] * 21, np.float32) + np.eye(6, dtype=np.float32)[np.triu_indices(6)] * 3.0),
                         rng.normal(size=6) * 0.3)
        T[i] = E
    batches.append(Batch("prior-T", sums[:k].copy(), n_pts[:k].copy(), T=T))
    return batches


def iteration_batches(seed=11):
    """The iteration logic: cnt == 0, it == max_iteration, |dfitness| exactly at the threshold (the test is strict), thresholds 0
    and inf, n_points 1 and around 2^24, and ~10k random (err, cnt, n) for the rounding of cnt / n and sqrtf(err / cnt)."""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(6, 6)); S = M @ M.T + np.eye(6)
    base = system(S, rng.normal(size=6) * 0.01)
    out = []

    def rows(cnts, errs):
        s = np.tile(base, (len(cnts), 1)); s[:, 28] = cnts; s[:, 27] = errs
        return s
    # cnt == 0 with a state that must survive untouched
    s = rows([0.0, 0.0, -0.0], [5.0, 0.0, 1.0])
    out.append(Batch("cnt0", s, np.array([10, 0, 7], np.uint32), fitness=np.full(3, 0.5, np.float32), rmse=np.full(3, 0.25, np.float32)))
    # it == max_iteration: scores updated, no solve
    s = rows([3.0, 100.0], [2.0, 1.0])
    out.append(Batch("max-iter", s, np.array([4, 1000], np.uint32), crit=(0.0, 0.0, 5), it=5))
    out.append(Batch("max-iter-0", s, np.array([4, 1000], np.uint32), crit=(0.0, 0.0, 0), it=0))
    # |dfitness| exactly equal to relative_fitness: fitness 3/4 from 0.5 -> df = 0.25 (exact); relative_rmse inf
    s = rows([3.0, 3.0], [0.0, 0.0])
    prev = np.array([0.5, 1.0], np.float32)                              # df = +0.25 and -0.25
    out.append(Batch("df-equal", s, np.array([4, 4], np.uint32), crit=(0.25, math.inf, 100), fitness=prev.copy()))
    out.append(Batch("df-below", s, np.array([4, 4], np.uint32), crit=(float(np.nextafter(np.float32(0.25), np.float32(1))), math.inf, 100),
                     fitness=prev.copy()))
    # relative_rmse exactly at |drmse| (rmse 0 -> 0.5: err/cnt = 0.25)
    s = rows([3.0], [0.75])
    out.append(Batch("dr-equal", s, np.array([4], np.uint32), crit=(math.inf, 0.5, 100)))
    out.append(Batch("dr-below", s, np.array([4], np.uint32), crit=(math.inf, float(np.nextafter(np.float32(0.5), np.float32(1))), 100)))
    # thresholds 0 (never) and inf (always, unless a score is NaN)
    s = rows([10.0, 10.0, 5.0], [1.0, -1.0, math.nan])
    out.append(Batch("thr-0", s, np.array([20, 20, 20], np.uint32), crit=(0.0, 0.0, 100)))
    out.append(Batch("thr-inf", s, np.array([20, 20, 20], np.uint32), crit=(math.inf, math.inf, 100)))
    # n_points 1 and around 2^24 (the uint -> float conversion rounds)
    n_edge = np.array([1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 7, 2 ** 32 - 1], np.uint32)
    s = rows([1.0, 12345.0, 16777215.0, 16777216.0, 3.0, 1e7, 1.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    out.append(Batch("n-edge", s, n_edge, crit=(0.0, 0.0, 1), it=1))
    # random (err, cnt, n): the rounding of cnt / n and sqrtf(err / cnt), stopped by it == max_iteration
    k = 10000
    n = rng.integers(1, 2 ** 25, k).astype(np.uint32)
    cnt = np.floor(rng.random(k) * n.astype(np.float64)) + 1.0
    err = (rng.random(k) * cnt * 10.0 ** rng.uniform(-8, 0, k))
    s = rows(cnt.astype(np.float32), err.astype(np.float32))
    out.append(Batch("scores", s, n, crit=(0.0, 0.0, 7), it=7))
    return out
