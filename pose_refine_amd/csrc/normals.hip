// normals.hip -- surface-normal agreement: on the inlier pixels of every rendered box of a batch (launch_render_boxes), the normal of the render
// estimated from its depth against the normal of the scene frame estimated the same way (include/pose_refine.h has the definition)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off like the rest: differences in 64-bit integers, the normals and their comparison in
// double in the header's operand order -- every decision is bit-identical to the CPU restatement (tests/normals_ref.py).
#include "score_walk.h"

namespace prk {

// a neighbour at distance h: usable when it holds a depth (n > 0) within `jump` of the centre's (64 bits: no overflow for any int32 pair)
__device__ __forceinline__ bool normal_neighbour_ok(int32_t c, int32_t n, int64_t jump)
{
    const int64_t diff = (int64_t)n - (int64_t)c;
    return n > 0 && diff <= jump && -diff <= jump;
}
// the unnormalised normal of a depth image at frame pixel (x, y), pointing away from the camera: centre z, neighbours l, r (x -+ h), u, d (y -+ h)
struct Normal3 { double a, b, c; };
__device__ __forceinline__ Normal3 depth_normal(const NormalParams &p, int x, int y, int32_t z, int32_t l, int32_t r, int32_t u, int32_t d)
{
    const double gu = (double)((int64_t)r - (int64_t)l), gv = (double)((int64_t)d - (int64_t)u);
    Normal3 n;
    n.a = -(p.fx * gu);
    n.b = -(p.fy * gv);
    n.c = ((double)(2 * p.step) * (double)z + ((double)x - p.cx) * gu) + ((double)y - p.cy) * gv;
    return n;
}
__device__ __forceinline__ double dot3(const Normal3 &u, const Normal3 &v) { return (u.a * v.a + u.b * v.b) + u.c * v.c; }

// The box walk of score_box_kernel: one workgroup = 16 image rows of one hypothesis' box, 4 wavefronts x 4 rows, lanes along a row, 64-column strips.
// Each lane reads its centre pixel and the four render neighbours at distance h from the packed box lines (they hit L1 / L2: no cross-lane
// exchange at a variable h) and the scene's centre pixel; a neighbour outside `win` {x0, row0, x1, row1} (the image the render lives in: the frame,
// or the ROI window, in image coordinates) or outside the packed box leaves the render normal undefined -- the first is outside the image, the
// second empty by construction.  Those six loads sit under no branch: a neighbour that does not exist is read at the centre's address and
// discarded, so all six are in flight together (with a branch around each, every one waited for its own round trip: 140 us instead of 93 for
// the 256 boxes of configs[1]; issuing two or four rows' loads together moves the call by 5 us either way: profiles/normals/README.md).  Only lanes on an inlier pixel (depth_class: pr_score_poses' test)
// with a defined render normal read the scene's four neighbours, for which the image is the whole frame.  Five counters per lane in registers,
// summed over the workgroup (block_totals), one integer atomic per non-zero counter and workgroup: exact and independent of chunking and batch
// composition.
template <typename SceneT>
__global__ __launch_bounds__(256) void normal_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                         const uint32_t *__restrict__ box_off, const int4 win, const SceneT *__restrict__ scene,
                                                         const NormalParams p, uint32_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63;
    BoxBlock blk;
    if (!box_block(bbox, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
    const int64_t t = p.tau, jump = p.jump;
    const int h = (int)p.step, W = (int)width, H = (int)height;
    // what a render neighbour must lie in: the box (a line to load from) and the image
    const int x_lo = max(bb.x, win.x), x_hi = min(bb.z, win.z), y_lo = max(r_lo, win.y), y_hi = min(r_hi, win.w);
    auto value = [](int32_t d) { return rendered(d) ? d : 0; };                         // nothing drawn -> empty
    uint32_t tested = 0, agree = 0, disagree = 0, no_r = 0, no_s = 0;
    for (int k = 0; k < 4; ++k) {
        const int row = row0 + k;                                   // the same for every lane of the wavefront
        if (row < r_lo || row > r_hi || row >= H) continue;
        const bool has_u = row - h >= y_lo, has_d = row + h <= y_hi, frame_y = row - h >= 0 && row + h < H;      // (the scene's image is the whole frame)
        const int32_t *mid = box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, (uint32_t)row, width, height);
        const int32_t *up = has_u ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, (uint32_t)(row - h), width, height) : mid;
        const int32_t *dn = has_d ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, (uint32_t)(row + h), width, height) : mid;
        const SceneT *srow = scene + (size_t)row * width;
        for (int x0 = bb.x; x0 <= bb.z && x0 < W; x0 += 64) {
            const int x = x0 + (int)lane;
            const bool in_x = x <= bb.z && x < W, has_l = in_x && x - h >= x_lo, has_r = in_x && x + h <= x_hi, frame_x = x - h >= 0 && x + h < W;
            const int xc = in_x ? x : x0, xl = has_l ? x - h : xc, xr = has_r ? x + h : xc;      // columns that exist, for every lane
            const int32_t c0 = mid[xc], s = (int32_t)srow[xc], l0 = mid[xl], r0 = mid[xr], u0 = up[xc], d0 = dn[xc];      // six loads in flight, none under a branch
            const int32_t c = in_x ? value(c0) : 0;
            const int32_t l = has_l ? value(l0) : 0, r = has_r ? value(r0) : 0, u = has_u ? value(u0) : 0, d = has_d ? value(d0) : 0;
            const bool inlier = c > 0 && depth_class(c, s, t) == 0;
            const bool r_ok = normal_neighbour_ok(c, l, jump) & normal_neighbour_ok(c, r, jump) & normal_neighbour_ok(c, u, jump) & normal_neighbour_ok(c, d, jump);
            const bool both = inlier & r_ok & frame_x & frame_y;   // ... and the scene's neighbours lie inside the frame
            no_r += inlier & !r_ok;
            no_s += inlier & r_ok & !both;
            if (!both) continue;
            const SceneT *sp = srow + x;
            const int32_t sl = (int32_t)sp[-h], sr = (int32_t)sp[h], su = (int32_t)(sp - (size_t)h * width)[0], sd = (int32_t)(sp + (size_t)h * width)[0];
            if (!(normal_neighbour_ok(s, sl, jump) & normal_neighbour_ok(s, sr, jump) & normal_neighbour_ok(s, su, jump) & normal_neighbour_ok(s, sd, jump))) { ++no_s; continue; }
            const Normal3 nr = depth_normal(p, x, row, c, l, r, u, d), ns = depth_normal(p, x, row, s, sl, sr, su, sd);
            const double dot = dot3(nr, ns), qr = dot3(nr, nr), qs = dot3(ns, ns);
            const bool ok = dot >= 0.0 && dot * dot >= p.m2 * (qr * qs);       // no square root, no division
            ++tested;
            agree += ok; disagree += !ok;
        }
    }
    const uint32_t cnt[5] = { tested, agree, disagree, no_r, no_s };
    const uint32_t sum = block_totals(cnt);                        // thread k < 5: the workgroup's total of counter k, 0 in every other thread
    if (sum) atomicAdd(records + (size_t)blockIdx.y * 8 + threadIdx.x, sum);
}

hipError_t launch_normal_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                               const void *scene, bool scene_i32, const NormalParams &p, uint32_t *records, hipStream_t s)
{
    return for_box_launches(depth, box_off, n_poses, width, height, scene, scene_i32, [&](const BoxLaunch &b, auto *sc) {
        hipLaunchKernelGGL(normal_box_kernel, b.grid, dim3(256), 0, s, b.depth, bbox + b.p0, width, height, b.box_off, window, sc, p, records + (size_t)b.p0 * 8);
    });
}

}  // namespace prk
