// cloud.h -- scenes from point clouds: THE definition of the k nearest neighbours of a scene point and of its PCA normal (include/pose_refine.h states
// it in words), one copy for the kernels of cloud.hip and the host twins of pr_cloud.cpp, and the launchers of cloud.hip.  The distances are float32
// without contraction (-ffp-contract=off), the normal is float64 in list order: device and host agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pr_internal.h"
#include "jacobi.h"

#if defined(__HIP__)
#define CLOUD_FN __host__ __device__ __forceinline__
#else
#define CLOUD_FN inline
#endif

namespace cloud {

static_assert(sizeof(pr_cloud_params) == 32 && sizeof(pr_cloud_counts) == 16, "pr_cloud_params / pr_cloud_counts layout");

// A tree as the walk sees it -- `Tree` is a small accessor over the node data (the derived traversal arrays on the device, the caller's pr_kdnode
// array on the host):
//   Topo  node(int)  const   the links of a node in SceneNNDev::topo's encoding: {split_v bits | left, child1 | right, child2 | -1, (parent + 1) | dim << 30}
//   Box   box(int)   const   a box that holds every point of the node's subtree
//   Point point(int) const   a scene point
// and a list -- `List` holds up to k (d2, j) pairs: float d(t), uint32_t j(t), void set(t, d2, j).
struct Topo { int x, y, z, w; };
struct Box { float lo[3], hi[3]; };
struct Point { float x, y, z; };

// d2(i, j): pcd_scene.h:88-91's expression and order, which IS the parity contract
CLOUD_FN float dist_sq(float sx, float sy, float sz, const Point &p)
{
    const float dx = p.x - sx, dy = p.y - sy, dz = p.z - sz;
    return (dx * dx + dy * dy) + dz * dz;
}
// distance of a query to a box: the terms added in dist_sq's order, each no larger than the term of any point inside the box -- a lower bound of
// the float32 d2 of every such point (rounding is monotonic), not merely of the real distance
CLOUD_FN float box_dist_sq(float sx, float sy, float sz, const Box &b)
{
    float lb = 0;
    if (sx < b.lo[0]) lb += (b.lo[0] - sx) * (b.lo[0] - sx); else if (sx > b.hi[0]) lb += (b.hi[0] - sx) * (b.hi[0] - sx);
    if (sy < b.lo[1]) lb += (b.lo[1] - sy) * (b.lo[1] - sy); else if (sy > b.hi[1]) lb += (b.hi[1] - sy) * (b.hi[1] - sy);
    if (sz < b.lo[2]) lb += (b.lo[2] - sz) * (b.lo[2] - sz); else if (sz > b.hi[2]) lb += (b.hi[2] - sz) * (b.hi[2] - sz);
    return lb;
}
// the order of the list: by distance, a tie to the lower index
CLOUD_FN bool key_less(float da, uint32_t ja, float db, uint32_t jb) { return da < db || (da == db && ja < jb); }

// (d2, j) into the ascending list of m <= k entries; returns the new m.  A full list takes the key only if it displaces the last entry.
template <class List>
CLOUD_FN uint32_t list_insert(List &l, uint32_t m, uint32_t k, float d2, uint32_t j)
{
    uint32_t t;
    if (m == k) {
        if (!key_less(d2, j, l.d(k - 1), l.j(k - 1))) return m;
        t = k - 1;
    } else t = m++;
    while (t > 0 && key_less(d2, j, l.d(t - 1), l.j(t - 1))) { l.set(t, l.d(t - 1), l.j(t - 1)); --t; }
    l.set(t, d2, j);
    return m;
}

// The ordered stackless walk of Scene_nn::query (nn_walk_stackless, nn_query.h) with `best` replaced by the list's bound: r2 until the list holds k
// entries, then the k-th d2.  A leaf point is tried iff d2 <= bound and a far child entered iff its box is within the bound -- both '<=', because an
// equal distance with a lower index still displaces.  Every point is met at most once and a subtree is skipped only when each of its points is
// strictly beyond the bound, so the list is the k smallest keys whatever the order of the visit.  Returns m.
template <class Tree, class List>
CLOUD_FN uint32_t knn_walk(const Tree &tree, List &list, uint32_t k, float r2, float sx, float sy, float sz)
{
    uint32_t m = 0;
    int cur = 0, prev = -1;
    bool climbing = false;
    float bound = r2;
    while (cur >= 0) {
        const Topo t = tree.node(cur);
        const int parent = (t.w & 0x3fffffff) - 1;
        if (!climbing && t.z < 0) {
            for (int i = t.x; i < t.y; ++i) {
                const float d2 = dist_sq(sx, sy, sz, tree.point(i));
                if (d2 <= bound) {
                    m = list_insert(list, m, k, d2, (uint32_t)i);
                    if (m == k) bound = list.d(k - 1);
                }
            }
            climbing = true; prev = cur; cur = parent;
            continue;
        }
        const int dim = (int)((uint32_t)t.w >> 30);
        const float q = (dim == 0) ? sx : ((dim == 1) ? sy : sz);
        float split;
        { const int bits = t.x; __builtin_memcpy(&split, &bits, sizeof split); }
        const float diff = q - split;
        const int near_c = (diff < 0) ? t.y : t.z;
        const int far_c  = (diff < 0) ? t.z : t.y;
        if (!climbing) { prev = cur; cur = near_c; continue; }
        if (prev == near_c) {
            const float lb = box_dist_sq(sx, sy, sz, tree.box(far_c));
            if (lb <= bound) { prev = cur; cur = far_c; climbing = false; continue; }
        }
        prev = cur; cur = parent;
    }
    return m;
}

// the normal of a point from its list: pose_refine.h's seven steps.  status: which of pr_cloud_counts' last three fields the point counts in
enum : uint32_t { kWithNormal = 0, kTooFew = 1, kDegenerate = 2 };
struct Normal { float n[3]; float variation; uint32_t status; };
template <class Tree, class List>
CLOUD_FN Normal normal_from_list(const Tree &tree, const List &list, uint32_t m, const pr_cloud_params &cp, float px, float py, float pz)
{
    Normal out = { { 0.0f, 0.0f, 0.0f }, 0.0f, kTooFew };
    if (m < cp.min_neighbours) return out;
    out.status = kDegenerate;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    for (uint32_t t = 0; t < m; ++t) {
        const Point p = tree.point((int)list.j(t));
        cx += (double)p.x; cy += (double)p.y; cz += (double)p.z;
    }
    const double md = (double)m;
    cx = cx / md; cy = cy / md; cz = cz / md;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (uint32_t t = 0; t < m; ++t) {
        const Point p = tree.point((int)list.j(t));
        const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    double A[3][3] = { { xx, xy, xz }, { xy, yy, yz }, { xz, yz, zz } };
    double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    (void)prr::jacobi_eigen<3>(A, V, PR_PLANE_MAX_SWEEPS);
    // lo / mid / hi by selects (no indexing by a variable: the matrices stay in registers on the device)
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    const int lo = (e1 < e0) ? ((e2 < e1) ? 2 : 1) : ((e2 < e0) ? 2 : 0);
    const int ra = (lo == 0) ? 1 : 0, rb = (lo == 2) ? 1 : 2;                    // the two that remain, in index order
    const double ea = (ra == 0) ? e0 : e1, eb = (rb == 1) ? e1 : e2;
    const double l_lo = (lo == 0) ? e0 : ((lo == 1) ? e1 : e2), l_mid = (eb < ea) ? eb : ea, l_hi = (eb < ea) ? ea : eb;
    if (l_mid <= (double)cp.line_ratio * l_hi) return out;
    double nx = (lo == 0) ? V[0][0] : ((lo == 1) ? V[0][1] : V[0][2]);
    double ny = (lo == 0) ? V[1][0] : ((lo == 1) ? V[1][1] : V[1][2]);
    double nz = (lo == 0) ? V[2][0] : ((lo == 1) ? V[2][1] : V[2][2]);
    const double vx = (double)cp.viewpoint[0] - (double)px, vy = (double)cp.viewpoint[1] - (double)py, vz = (double)cp.viewpoint[2] - (double)pz;
    if ((nx * vx + ny * vy) + nz * vz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    out.n[0] = (float)nx; out.n[1] = (float)ny; out.n[2] = (float)nz;
    out.variation = (float)(l_lo / ((l_lo + l_mid) + l_hi));
    out.status = kWithNormal;
    return out;
}

}  // namespace cloud

namespace prk {

constexpr uint32_t kCloudThreads = 128;                           // lanes of a workgroup of the walk: k KiB of LDS for the lists
constexpr uint32_t kCloudChunk = 1024;                            // samples per wavefront of the PPF gather

// cloud.hip.  One lane per scene point; any output pointer may be null.  idx / d2: n * k, count / variation: n, normal: n (may be tree.normal),
// tally: three words, zero on entry, the points per cloud::k* status (normal != null only).
hipError_t launch_cloud_knn(const SceneNNDev &tree, uint32_t n, const pr_cloud_params &cp, uint32_t *idx, float *d2, uint32_t *count, pr_vec3 *normal,
                            float *variation, uint32_t *tally, hipStream_t s);
// the samples 0, stride, 2 stride, ... with a normal: counts per chunk of kCloudChunk samples and their offsets (chunk_off[n_chunks] = the total), then the emit
hipError_t launch_cloud_sample_count(const pr_vec3 *normal, uint32_t n, uint32_t stride, uint32_t *chunk_count, uint32_t *chunk_off, hipStream_t s);
hipError_t launch_cloud_sample_emit(const pr_vec3 *pcd, const pr_vec3 *normal, uint32_t n, uint32_t stride, const uint32_t *chunk_off, pr_vec3 *points,
                                    pr_vec3 *normals, hipStream_t s);

}  // namespace prk
