// ppf.h -- point-pair features: THE definition of frame, feature key, pair angle and vote bin (include/pose_refine.h states it in words), one copy
// for the kernels of ppf.hip and the host code of pr_ppf.cpp, and the launchers of ppf.hip.  float32, no contraction (-ffp-contract=off), + - * /
// and sqrtf only: device and host agree bit for bit.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "pr_internal.h"

#if defined(__HIP__)
#define PPF_FN __host__ __device__ __forceinline__
#else
#define PPF_FN inline
#endif

namespace ppf {

// what the per-pair path reads of a pr_ppf_params: its float32 head (the double bin centres behind it are the host pose formula's)
struct Tables {
    float    diameter, dist_step, inv_dist_step;
    uint32_t n_dist, n_angle, n_alpha, n_keys, flip_model_normals;
    float    cos_edge[PR_PPF_MAX_ANGLE_BINS + 1];
    float    alpha_edge[PR_PPF_MAX_ALPHA_BINS / 2 + 1];
};
static_assert(sizeof(Tables) == 296 && sizeof(pr_ppf_params) == 1320, "Tables is the head of pr_ppf_params");
static_assert(sizeof(pr_ppf_entry) == 12 && sizeof(pr_ppf_peak) == 16, "pr_ppf_entry / pr_ppf_peak layout");

PPF_FN float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
PPF_FN bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }            // false for NaN and the infinities
PPF_FN bool good_len(float v) { return v > 0.0f && v <= FLT_MAX; }

struct Frame { float ux, uy, uz, vx, vy, vz; bool ok; };
PPF_FN Frame make_frame(float nx, float ny, float nz)
{
    const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    float wx, wy, wz;
    if (ax <= ay && ax <= az) { wx = 0.0f; wy = -nz; wz = ny; }           // e = x
    else if (ay <= az)        { wx = nz; wy = 0.0f; wz = -nx; }           // e = y
    else                      { wx = -ny; wy = nx; wz = 0.0f; }           // e = z
    const float l = sqrtf(dot3(wx, wy, wz, wx, wy, wz));
    Frame f;
    f.ok = good_len(l);
    f.ux = wx / l; f.uy = wy / l; f.uz = wz / l;
    f.vx = ny * f.uz - nz * f.uy; f.vy = nz * f.ux - nx * f.uz; f.vz = nx * f.uy - ny * f.ux;
    return f;
}

// the number of k in 1 .. n-1 with c <= edge[k]
PPF_FN uint32_t edge_bin(const float *edge, uint32_t n, float c)
{
    uint32_t b = 0;
    for (uint32_t k = 1; k < n; ++k) b += (c <= edge[k]) ? 1u : 0u;
    return b;
}

struct Pair { uint32_t key; float c, s; bool ok; };
// reference (pr, nr) with its frame, other point (pi, ni); cos_edge: the descriptor's table (or a copy of it)
PPF_FN Pair make_pair(const Frame &fr, float inv_dist_step, uint32_t n_dist, uint32_t n_angle, const float *cos_edge, const pr_vec3 pr, const pr_vec3 nr,
                      const pr_vec3 pi, const pr_vec3 ni)
{
    Pair p; p.key = 0; p.c = p.s = 0.0f; p.ok = false;
    const float dx = pi.x - pr.x, dy = pi.y - pr.y, dz = pi.z - pr.z;
    const float L = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    if (!fr.ok || !good_len(L)) return p;
    const float t = L * inv_dist_step;
    if (!(t < (float)n_dist)) return p;
    const float c1 = dot3(nr.x, nr.y, nr.z, dx, dy, dz) / L, c2 = dot3(ni.x, ni.y, ni.z, dx, dy, dz) / L, c3 = dot3(nr.x, nr.y, nr.z, ni.x, ni.y, ni.z);
    if (!finite_f(c1) || !finite_f(c2) || !finite_f(c3)) return p;
    const float y = dot3(dx, dy, dz, fr.ux, fr.uy, fr.uz), z = dot3(dx, dy, dz, fr.vx, fr.vy, fr.vz);
    const float r = sqrtf(y * y + z * z);
    if (!good_len(r)) return p;
    p.c = y / r; p.s = z / r;
    const uint32_t bd = (uint32_t)(int)t;
    p.key = ((bd * n_angle + edge_bin(cos_edge, n_angle, c1)) * n_angle + edge_bin(cos_edge, n_angle, c2)) * n_angle + edge_bin(cos_edge, n_angle, c3);
    p.ok = true;
    return p;
}

// the bin of (scene angle) - (model angle), or -1: no vote
PPF_FN int alpha_bin(const float *alpha_edge, uint32_t n_alpha, float cs, float ss, float cm, float sm)
{
    const float ca = cs * cm + ss * sm, sa = ss * cm - cs * sm;
    const float q = sqrtf(ca * ca + sa * sa);
    if (!good_len(q)) return -1;
    const uint32_t h = edge_bin(alpha_edge, n_alpha / 2, ca / q);
    return (int)(sa >= 0.0f ? h : n_alpha - 1 - h);
}

}  // namespace ppf

namespace prk {

// ppf.hip.  counts: n_keys words of scratch (the histogram, then the per-bucket cursors); offsets: n_keys + 1 words
hipError_t launch_ppf_model_build(const ppf::Tables &tb, const pr_vec3 *points, const pr_vec3 *normals, uint32_t n_model, uint32_t *counts,
                                  uint32_t *offsets, pr_ppf_entry *entries, hipStream_t s);
// gh = ceil(height / stride) sampled rows: row_count[gh], row_off[gh + 1] (the last word: the total)
hipError_t launch_ppf_scene_count(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, uint32_t *row_count,
                                  uint32_t *row_off, hipStream_t s);
hipError_t launch_ppf_scene_emit(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, const uint32_t *row_off,
                                 pr_vec3 *points, pr_vec3 *normals, hipStream_t s);
struct PpfRef { pr_vec3 p, n; };             // a reference as the vote kernel read it (for the host's pose formula)
hipError_t launch_ppf_vote(const ppf::Tables &tb, const uint32_t *offsets, const pr_ppf_entry *entries, uint32_t n_model, const pr_vec3 *points,
                           const pr_vec3 *normals, uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks,
                           pr_ppf_peak *peaks, PpfRef *refs, uint32_t *acc_out, bool cooperative, hipStream_t s);
// pr_ppf_vote_multi: one model of the table as the kernel reads it (staged per call: pinned block -> device by launch_stage_words, whole 16-byte words)
struct PpfModelRec {
    ppf::Tables tb;
    const uint32_t *offsets; const pr_ppf_entry *entries;
    uint32_t n_model, peak_base;             // peak_base: the model's first peak, = its index in the caller's table * n_refs * n_peaks (the rows of the launch are in another order)
    uint64_t acc_base;                       // the model's first accumulator word: n_refs * the cells of the models before it
    uint64_t pad;
};
static_assert(sizeof(PpfModelRec) == 336 && sizeof(PpfModelRec) % 16 == 0, "PpfModelRec: whole 16-byte words");
// grid (n_refs, n_models); max_cells: the largest n_model * n_alpha of the table (the launch's dynamic LDS); refs: n_refs records, written once
hipError_t launch_ppf_vote_multi(const PpfModelRec *models, uint32_t n_models, uint32_t max_cells, const pr_vec3 *points, const pr_vec3 *normals, uint32_t n_scene,
                                 uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks, PpfRef *refs, uint32_t *acc_out,
                                 bool cooperative, hipStream_t s);

}  // namespace prk
