// vsd.hip -- visible surface discrepancy: the depth boxes of TWO renders of a rendered batch (launch_render_boxes), an estimate and a truth,
// against one scene depth frame; integer counts per pair (pr_vsd_counts)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off, '/' and sqrtf correctly rounded: every per-pixel value is bit-identical to the
// numpy float32 restatement (tests/vsd_ref.py).
#include "score_walk.h"

namespace prk {

// The two visibility masks and their combination for one frame pixel (include/pose_refine.h, pr_pose_vsd): e, g = the two renders' values (0:
// nothing drawn), s = the scene value, c = the pixel's ray factor.  Returns bit 0 = vg, bit 1 = ve; *ad = |G - E| (meaningful where both are set).
__device__ __forceinline__ uint32_t vsd_pixel(int32_t e, int32_t g, int32_t s, float c, float delta, float *ad)
{
    const float E = e > 0 ? (float)e * c : 0.0f;
    const float G = g > 0 ? (float)g * c : 0.0f;
    const float T = s > 0 ? (float)s * c : 0.0f;
    const bool vg = G > 0.0f && (T == 0.0f || G - T <= delta);
    const bool ve = E > 0.0f && (T == 0.0f || E - T <= delta || vg);
    *ad = fabsf(G - E);
    return (vg ? 1u : 0u) | (ve ? 2u : 0u);
}

// One workgroup = 16 image rows of one PAIR (score_box_kernel's shape: 4 wavefronts x 4 rows, lanes along a row, 256 columns per step), over the
// bounding box of the union of the pair's two pixel boxes.  A render is addressed (box_line) only inside its own box and is "nothing drawn"
// outside it; the scene value is read from the same frame pixel.  All 48 loads of a step are issued before the first compare.  The sixteen
// counters stay in registers, go through block_totals and end in one integer atomic per non-zero counter and workgroup: exact in any order.
// A lane sees at most 4 rows x 128 columns per counter (frames <= 8192 wide): no counter can overflow before the atomics.
template <typename SceneT>
__global__ __launch_bounds__(256) void vsd_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                      const uint32_t *__restrict__ box_off, const SceneT *__restrict__ scene, VsdParams pm,
                                                      VsdPairing pairing, uint32_t pair0, uint32_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t pair = pair0 + blockIdx.y;
    const uint32_t pe = pair * pairing.est_mul, pg = pair * pairing.gt_mul + pairing.gt_add;
    const int4 be = bbox[pe], bg = bbox[pg];
    const bool has_e = be.x <= be.z && be.y <= be.w, has_g = bg.x <= bg.z && bg.y <= bg.w;
    int4 bu = has_e ? be : bg;                                      // both empty: an empty box, box_block says no
    if (has_e && has_g) bu = make_int4(min(be.x, bg.x), min(be.y, bg.y), max(be.z, bg.z), max(be.w, bg.w));
    BoxBlock blk;
    if (!box_block(bu, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
    // each render's own image rows (raster rows run flipped); an empty box has none
    const int e_lo = has_e ? (int)height - 1 - be.w : 1, e_hi = has_e ? (int)height - 1 - be.y : 0;
    const int g_lo = has_g ? (int)height - 1 - bg.w : 1, g_hi = has_g ? (int)height - 1 - bg.y : 0;
    const bool has_k = pm.has_k != 0;
    uint32_t cnt[4] = { 0, 0, 0, 0 }, far[PR_VSD_MAX_TAUS];
#pragma unroll
    for (uint32_t k = 0; k < PR_VSD_MAX_TAUS; ++k) far[k] = 0;
    float yy[4];                                                    // yn * yn of this wavefront's four rows
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const float yn = ((float)(row0 + (int)r) - pm.cy) / pm.fy;
        yy[r] = has_k ? yn * yn : 0.0f;
    }
    for (int x0 = bb.x; x0 <= bb.z; x0 += 256) {
        int32_t ev[4][4], gv[4][4], sv[4][4];                       // 48 loads in flight per lane before the first compare
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const int row = row0 + (int)r;
            const bool live = row < (int)height && row >= r_lo && row <= r_hi;
            const bool live_e = live && row >= e_lo && row <= e_hi, live_g = live && row >= g_lo && row <= g_hi;
            const int32_t *le = live_e ? box_line(const_cast<int32_t *>(depth), box_off, be, pe, (uint32_t)row, width, height) : depth;
            const int32_t *lg = live_g ? box_line(const_cast<int32_t *>(depth), box_off, bg, pg, (uint32_t)row, width, height) : depth;
            const SceneT *srow = scene + (live ? (size_t)row * width : 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + 64 * j + (int)lane;
                const bool in = live && x <= bb.z;
                const bool in_e = live_e && x >= be.x && x <= be.z, in_g = live_g && x >= bg.x && x <= bg.z;
                ev[r][j] = in_e ? le[x] : 0;
                gv[r][j] = in_g ? lg[x] : 0;
                sv[r][j] = in ? (int32_t)srow[x] : 0;
            }
        }
        float xx[4];                                                // xn * xn of this lane's four columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xn = ((float)(x0 + 64 * j + (int)lane) - pm.cx) / pm.fx;
            xx[j] = has_k ? xn * xn : 0.0f;
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t e = rendered(ev[r][j]) ? ev[r][j] : 0, g = rendered(gv[r][j]) ? gv[r][j] : 0;
                if (e == 0 && g == 0) continue;
                const float c = has_k ? sqrtf((xx[j] + yy[r]) + 1.0f) : 1.0f;
                float ad;
                const uint32_t m = vsd_pixel(e, g, sv[r][j], c, pm.delta, &ad);
                cnt[0] += m & 1u; cnt[1] += m >> 1; cnt[2] += m == 3u; cnt[3] += m != 0u;
                if (m == 3u) {
#pragma unroll
                    for (uint32_t k = 0; k < PR_VSD_MAX_TAUS; ++k)
                        if (k < pm.n_taus) far[k] += ad >= pm.tau[k];
                }
            }
    }
    uint32_t v[4 + PR_VSD_MAX_TAUS];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v[k] = cnt[k];
#pragma unroll
    for (uint32_t k = 0; k < PR_VSD_MAX_TAUS; ++k) v[4 + k] = far[k];
    const uint32_t sum = block_totals(v);
    if (threadIdx.x < 4 + PR_VSD_MAX_TAUS && sum) atomicAdd(records + (size_t)pair * (4 + PR_VSD_MAX_TAUS) + threadIdx.x, sum);
}

hipError_t launch_vsd_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_pairs, const VsdPairing &pairing, uint32_t width,
                            uint32_t height, const void *scene, bool scene_i32, const VsdParams &pm, uint32_t *records, hipStream_t s)
{
    for (uint32_t p0 = 0; p0 < n_pairs; p0 += 32768) {              // grid.y is limited to 65535 (for_box_launches)
        const uint32_t np = (n_pairs - p0 < 32768) ? (n_pairs - p0) : 32768;
        const dim3 grid((height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np);
        with_scene(scene, scene_i32, [&](auto *sc) {
            hipLaunchKernelGGL(vsd_box_kernel, grid, dim3(256), 0, s, depth, bbox, width, height, box_off, sc, pm, pairing, p0, records);
        });
    }
    return hipGetLastError();
}

}  // namespace prk
