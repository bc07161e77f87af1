// pose_box.h -- the conservative pixel box of a mesh under one pose.  The same source is compiled for the device (pose_bbox_kernel,
// pose_bbox_multi_kernel: PR_HD = __host__ __device__) and for the host (the asynchronous path sizes a batch with it before anything of
// the batch has run); with contraction disabled both builds produce the same box.  Also the hash of one triangle, which the host (fingerprint of a
// triangle buffer, taken when its ordered copy is made) and the raster's per-batch check of the caller's buffer must form alike.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>

#include "pr_internal.h"

#ifndef PR_HD
#define PR_HD
#define PR_HD_HOST_ONLY 1                                            // (a host translation unit: no device intrinsics below, even in its device pass)
#endif

namespace prk {

// {x0,y0,x1,y1} (raster coordinates, y not yet flipped) of the mesh box `aabb` {minx,miny,minz,maxx,maxy,maxz} under the model matrix M:
// the 8 box corners go through the same model / projection / viewport arithmetic as the vertices; the projection of any point of the box
// lies in the hull of the projected corners as long as all of them are in front of the camera, and 2 pixels of padding cover float
// rounding.  Any corner at or behind the camera plane -> the whole frame.
PR_HD inline int4 pose_pixel_box(const float *aabb, const float *M, const pr_mat4 &proj, uint32_t width, uint32_t height, pr_roi roi)
{
    float mnx = FLT_MAX, mny = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX;
    bool all_front = true;
    for (int c = 0; c < 8; ++c) {
        const float x = aabb[(c & 1) ? 3 : 0], y = aabb[(c & 2) ? 4 : 1], z = aabb[(c & 4) ? 5 : 2];
        const float lx = M[0] * x + M[1] * y + M[2] * z + M[3];
        const float ly = M[4] * x + M[5] * y + M[6] * z + M[7];
        const float lz = M[8] * x + M[9] * y + M[10] * z + M[11];
        if (!(lz > 1e-3f)) all_front = false;
        const float cxp = proj.m[0] * lx + proj.m[1] * ly + proj.m[2] * lz + proj.m[3];
        const float cyp = proj.m[4] * lx + proj.m[5] * ly + proj.m[6] * lz + proj.m[7];
        const float sx = cxp / lz * (float)width / 2.0f + (float)width / 2.0f;
        const float sy = cyp / lz * (float)height / 2.0f + (float)height / 2.0f;
        mnx = fminf(mnx, sx); mxx = fmaxf(mxx, sx); mny = fminf(mny, sy); mxy = fmaxf(mxy, sy);
    }
    auto imax = [](int a, int b) { return a > b ? a : b; };
    auto imin = [](int a, int b) { return a < b ? a : b; };
    int x0 = 0, y0 = 0, x1 = (int)width - 1, y1 = (int)height - 1;
    const bool finite = (mnx > -1e8f) && (mxx < 1e8f) && (mny > -1e8f) && (mxy < 1e8f);
    if (all_front && finite) {
        x0 = imax(0, (int)floorf(mnx) - 2);  x1 = imin((int)width - 1, (int)ceilf(mxx) + 2);
        y0 = imax(0, (int)floorf(mny) - 2);  y1 = imin((int)height - 1, (int)ceilf(mxy) + 2);
    }
    if (roi.width > 0 && roi.height > 0) {                       // renderer.cu:106-113: the ROI is given in image rows, the raster runs flipped
        x0 = imax(x0, roi.x);  x1 = imin(x1, roi.x + roi.width - 1);
        y0 = imax(y0, (int)height - 1 - (roi.y + roi.height - 1));  y1 = imin(y1, (int)height - 1 - roi.y);
    }
    return make_int4(x0, y0, x1, y1);
}

// ---- the packed layouts of a (sub-)batch: THE definition, for the host that sizes and stages a batch and for the kernels that form the same
// offsets on the device (box_pack_offsets_kernel, d2c_pack_starts_kernel) -- the two must agree byte for byte.  A pixel box is its own little
// image of box_area ints in the depth workspace, a cloud a run of points; each starts where the one before it ends, rounded up to kBoxPack
// ints / kCloudAlign points (128-byte lines).  An empty or inverted box (an off-screen pose) has no pixels.
static_assert(kCloudAlign > 0 && (kCloudAlign & (kCloudAlign - 1)) == 0, "kCloudAlign: a power of two");
static_assert(kBoxPack > 0 && (kBoxPack & (kBoxPack - 1)) == 0, "kBoxPack: a power of two");
PR_HD inline uint32_t box_area(const int4 b)
{
    const int w = b.z - b.x + 1, h = b.w - b.y + 1;
    return (uint32_t)(w > 0 ? w : 0) * (uint32_t)(h > 0 ? h : 0);
}
PR_HD inline uint32_t box_slot(uint32_t area) { return (area + (kBoxPack - 1u)) & ~(kBoxPack - 1u); }
PR_HD inline uint32_t cloud_slot(uint32_t count) { return (count + (kCloudAlign - 1u)) & ~(kCloudAlign - 1u); }

// ---- the BANDED layout of a depth box (asynchronous fused path, option box_bands): four consecutive image rows interleaved column by column, so
// that a 64-byte segment holds a 4x4-pixel patch instead of 16 pixels of one row -- the raster's depth atomics cost one request per distinct
// segment a wave instruction addresses, and the ~30 small triangles a wavefront drains together cover a patch a few pixels high.  Bands are
// aligned to IMAGE rows (multiples of 4: a wavefront of the box walks owns exactly one), not to the box: box `b` (inclusive, raster y) of a
// frame `height` rows high has image rows r0 = height - 1 - b.w .. r1 = height - 1 - b.y, its first band starts at R = r0 & ~3 and it has
// nb = ((r1 | 3) - R + 1) / 4 bands of 4 * w ints, w = its width (no padding).  The up to 3 + 3 rows of the first and last band that lie outside the
// box hold "nothing drawn" like any pixel no fragment reached, and no fragment addresses them.
//   Capacity: R >= 0 and (r1 | 3) + 1 <= (height + 3) & ~3, so a box never needs more than width * ((height + 3) & ~3) ints (+ kBoxPack of rounding:
// the workspace bound per hypothesis).  A box inside another (the tight box inside the loose one) has r0' >= r0, r1' <= r1, hence R' >= R,
// (r1' | 3) <= (r1 | 3) and nb' <= nb, with w' <= w: its slot is never larger, so every offset and capacity derived from the loose boxes holds.
struct BandBox { int w, r0, R; uint32_t nb; };                       // (an empty or inverted box: w = 0, nb = 0)
PR_HD inline BandBox band_box(const int4 b, uint32_t height)
{
    BandBox k{ 0, 0, 0, 0u };
    const int w = b.z - b.x + 1, h = b.w - b.y + 1;
    if (w <= 0 || h <= 0) return k;
    const int r1 = (int)height - 1 - b.y;
    k.w = w; k.r0 = (int)height - 1 - b.w; k.R = k.r0 & ~3;
    k.nb = (uint32_t)(((r1 | 3) - k.R + 1) / 4);
    return k;
}
// ints a box occupies before rounding, in either layout, and its slot
PR_HD inline uint32_t box_ints(const int4 b, uint32_t height, bool bands)
{
    if (!bands) return box_area(b);
    const BandBox k = band_box(b, height);
    return 4u * (uint32_t)k.w * k.nb;
}
PR_HD inline uint32_t box_slot_of(const int4 b, uint32_t height, bool bands) { return box_slot(box_ints(b, height, bands)); }
// The constant part of a banded address: pixel (x, image row r) of box `b` lives at band_origin + band_index(w, x, r) ints from the box's
// offset -- i.e. at (((r >> 2) - (R >> 2)) * w + (x - b.x)) * 4 + (r & 3).  The raster folds offset + origin into one scalar base.
PR_HD inline ptrdiff_t band_origin(const BandBox &k, const int4 b) { return -(((ptrdiff_t)(k.R >> 2) * k.w + b.x) * 4); }
PR_HD inline uint32_t band_index(uint32_t w, uint32_t x, uint32_t r)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(PR_HD_HOST_ONLY)
    return ((__umul24(r >> 2, w) + x) << 2) | (r & 3u);          // a frame side is at most 8192 (frame_size_ok): exact, and full rate where v_mul_lo_u32 is a quarter
#else
    return (((r >> 2) * w + x) << 2) | (r & 3u);
#endif
}
PR_HD inline uint32_t band_pixel_offset(const int4 b, uint32_t height, int x, int r)
{
    const BandBox k = band_box(b, height);
    return (uint32_t)(band_origin(k, b) + (ptrdiff_t)band_index((uint32_t)k.w, (uint32_t)x, (uint32_t)r));
}
// the same for the row-major box (box_line, pr_device.h): pitch = the box's width, origin at its top-left pixel
PR_HD inline uint32_t row_pixel_offset(const int4 b, uint32_t height, int x, int r)
{
    const int w = b.z - b.x + 1;
    return (uint32_t)((r - ((int)height - 1 - b.w)) * (w > 0 ? w : 0) + (x - b.x));
}

// One vertex to the screen: model transform (renderer.h:296-303 mat_mul_v, rows a,b,c), projection rows 0 and 1 (only x and y of the result are
// used downstream), viewport (renderer.cu:90-98).  THE definition: the raster's triangle setup and the tight pixel box (below) both call it, so with
// contraction disabled the box is formed from the very floats the raster loops over.
struct ScreenVertex { float px, py, lz; };
PR_HD inline ScreenVertex vertex_to_screen(float x, float y, float z, const float *M, const pr_mat4 &proj, uint32_t width, uint32_t height)
{
    const float lx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const float ly = M[4] * x + M[5] * y + M[6] * z + M[7];
    const float lz = M[8] * x + M[9] * y + M[10] * z + M[11];
    const float cxp = proj.m[0] * lx + proj.m[1] * ly + proj.m[2] * lz + proj.m[3];
    const float cyp = proj.m[4] * lx + proj.m[5] * ly + proj.m[6] * lz + proj.m[7];
    ScreenVertex s;
    s.px = cxp / lz * (float)width / 2.0f + (float)width / 2.0f;
    s.py = cyp / lz * (float)height / 2.0f + (float)height / 2.0f;
    s.lz = lz;
    return s;
}

// The tight pixel box of a hypothesis: the hull of the mesh's projected VERTICES instead of the projected corners of its box (the fused
// asynchronous path, option tight_box).  TightAcc is what a pass over the vertices keeps -- running bounds of px / py and whether any vertex
// is unusable: at or behind the camera plane, or with a coordinate that is not finite (NaN never enters fminf / fmaxf, so it is counted here).
// Minima and maxima are exact in any order: every split of the vertices over lanes, merged in any tree, gives the same TightAcc.
struct TightAcc { float mnx, mny, mxx, mxy; uint32_t bad; };
PR_HD inline TightAcc tight_acc_empty() { return TightAcc{ FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, 0u }; }
PR_HD inline void tight_acc_add(TightAcc &a, const ScreenVertex &s)
{
    if (!(s.lz > 1e-3f) || !(fabsf(s.px) < 1e8f) || !(fabsf(s.py) < 1e8f)) a.bad = 1u;
    a.mnx = fminf(a.mnx, s.px); a.mxx = fmaxf(a.mxx, s.px); a.mny = fminf(a.mny, s.py); a.mxy = fmaxf(a.mxy, s.py);
}
PR_HD inline void tight_acc_merge(TightAcc &a, const TightAcc &b)
{
    a.mnx = fminf(a.mnx, b.mnx); a.mxx = fmaxf(a.mxx, b.mxx); a.mny = fminf(a.mny, b.mny); a.mxy = fmaxf(a.mxy, b.mxy); a.bad |= b.bad;
}
// ... and the box it stands for: pose_pixel_box's rounding and padding ({floor(min) - 2, ceil(max) + 2}), intersected with the LOOSE box
// `loose` (pose_pixel_box: it carries the frame and ROI clamps), so the result is never larger than the box everything was sized with.  An
// unusable vertex, or no vertex at all, leaves the hypothesis on its loose box.
PR_HD inline int4 tight_pixel_box(const TightAcc &a, const int4 loose)
{
    if (a.bad || !(a.mnx <= a.mxx) || !(a.mny <= a.mxy)) return loose;
    auto imax = [](int p, int q) { return p > q ? p : q; };
    auto imin = [](int p, int q) { return p < q ? p : q; };
    return make_int4(imax(loose.x, (int)floorf(a.mnx) - 2), imax(loose.y, (int)floorf(a.mny) - 2),
                     imin(loose.z, (int)ceilf(a.mxx) + 2), imin(loose.w, (int)ceilf(a.mxy) + 2));
}

// Mixing hash of one triangle's nine words (bit patterns: -0.0f and 0.0f, or two NaNs, are different content).  The fingerprint of a
// triangle buffer is the wrapping 64-bit SUM of these over its triangles -- a multiset hash, equal for every order of the same triangles --
// so the host (when it builds the ordered copy) and the raster's per-batch check (over the caller's buffer, in whatever order the
// workgroups arrive) form the same number.
PR_HD inline unsigned long long triangle_hash(const uint32_t (&w)[9])
{
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < 9; ++k) { h = (h ^ w[k]) * 0xff51afd7ed558ccdull; h ^= h >> 32; }
    h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 29);
}

}  // namespace prk
