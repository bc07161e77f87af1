// contour.hip -- depth-edge (contour) agreement: the scene's edge pixels with their chessboard distance transform and their nearest-edge map
// (contour_fit.hip's input), each made once per frame, and the edge pixels of every rendered box of a batch (launch_render_boxes) counted against
// the distance transform
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off like the rest (integer arithmetic only: differences in 64 bits).
#include "score_walk.h"

namespace prk {

// ---- scene side: three launches ---------------------------------------------------------------------------------------------------
// (1) edge bits.  One wavefront per 64-pixel word of a row: bit b of word w of row y is frame pixel (64 w + b, y), 0 beyond the row's end.
template <typename SceneT>
__global__ __launch_bounds__(256) void scene_edge_kernel(const SceneT *__restrict__ scene, uint32_t width, uint32_t height, int32_t jump_mm,
                                                         unsigned long long *__restrict__ bits, uint32_t words_per_row)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cell = blockIdx.x * 4 + (threadIdx.x >> 6);     // (row, word): the same for every lane of the wavefront
    if (cell >= height * words_per_row) return;
    const uint32_t y = cell / words_per_row, w = cell - y * words_per_row, x = 64 * w + lane;
    const int64_t jump = jump_mm;
    bool edge = false;
    if (x < width) {
        const SceneT *row = scene + (size_t)y * width;
        const int32_t c = (int32_t)row[x];
        if (c > 0) {
            auto at = [&](const SceneT *r, uint32_t xx) { const int32_t v = (int32_t)r[xx]; return v > 0 ? v : 0; };
            const int32_t l = x > 0 ? at(row, x - 1) : kNoNeighbour, r = x + 1 < width ? at(row, x + 1) : kNoNeighbour;
            const int32_t u = y > 0 ? at(row - width, x) : kNoNeighbour, d = y + 1 < height ? at(row + width, x) : kNoNeighbour;
            edge = edge_trigger(c, l, jump) || edge_trigger(c, r, jump) || edge_trigger(c, u, jump) || edge_trigger(c, d, jump);
        }
    }
    const unsigned long long m = __ballot(edge);
    if (lane == 0) bits[cell] = m;
}

// The distances from pixel x to the nearest edge pixel of its row at or left of it (dl) and at or right of it (dr), 64 when the pixel's own word and
// one word on either side hold none (radius <= 32: they hold every candidate).  right: bit k = pixel x + k; left: bit 63 - k = pixel x - k.
__device__ __forceinline__ void row_edge_distances(const unsigned long long *__restrict__ brow, uint32_t x, uint32_t words_per_row, uint32_t &dl, uint32_t &dr)
{
    const uint32_t w = x >> 6, b = x & 63;
    const unsigned long long here = brow[w], prev = w > 0 ? brow[w - 1] : 0ull, next = w + 1 < words_per_row ? brow[w + 1] : 0ull;
    const unsigned long long right = (here >> b) | (b ? next << (64 - b) : 0ull);
    const unsigned long long left = (here << (63 - b)) | (b < 63 ? prev >> (b + 1) : 0ull);
    dr = right ? (uint32_t)__builtin_ctzll(right) : 64u;
    dl = left ? (uint32_t)__builtin_clzll(left) : 64u;
}

// (2) distance along the row to the nearest edge pixel, 255 beyond `radius`
__global__ __launch_bounds__(256) void edge_row_dist_kernel(const unsigned long long *__restrict__ bits, uint32_t width, uint32_t height, uint32_t words_per_row,
                                                            uint32_t radius, uint8_t *__restrict__ row_dist)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    uint32_t dl, dr;
    row_edge_distances(bits + (size_t)y * words_per_row, x, words_per_row, dl, dr);
    const uint32_t d = dr < dl ? dr : dl;
    row_dist[(size_t)y * width + x] = (uint8_t)(d <= radius ? d : 255u);
}

// (3) D(x, y) = min over |dy| <= radius of max(|dy|, row distance at (x, y + dy)): the chessboard distance, exact; 255 when none is within radius.
__global__ __launch_bounds__(256) void edge_col_dist_kernel(const uint8_t *__restrict__ row_dist, uint32_t width, uint32_t height, uint32_t radius,
                                                            uint8_t *__restrict__ dist)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const int y_lo = max((int)y - (int)radius, 0), y_hi = min((int)y + (int)radius, (int)height - 1);
    uint32_t best = 255;
    for (int yy = y_lo; yy <= y_hi; ++yy) {
        const uint32_t dy = (uint32_t)(yy > (int)y ? yy - (int)y : (int)y - yy), rd = row_dist[(size_t)yy * width + x];
        const uint32_t d = rd > dy ? rd : dy;                       // rd == 255: no candidate in that row
        best = d < best ? d : best;
    }
    dist[(size_t)y * width + x] = (uint8_t)best;
}

hipError_t launch_scene_edge_distance(const void *scene, bool scene_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                                      unsigned long long *bits, uint8_t *row_dist, uint8_t *dist, hipStream_t s)
{
    const uint32_t wpr = overlap_words_per_row(width), cells = height * wpr;       // frames hold at most 2^24 pixels
    with_scene(scene, scene_i32, [&](auto *sc) { hipLaunchKernelGGL(scene_edge_kernel, dim3((cells + 3) / 4), dim3(256), 0, s, sc, width, height, jump_mm, bits, wpr); });
    const dim3 grid((width + 255) / 256, height);                   // height <= 8192
    hipLaunchKernelGGL(edge_row_dist_kernel, grid, dim3(256), 0, s, bits, width, height, wpr, radius, row_dist);
    hipLaunchKernelGGL(edge_col_dist_kernel, grid, dim3(256), 0, s, row_dist, width, height, radius, dist);
    return hipGetLastError();
}

// ---- the nearest scene edge pixel (pr_scene_edge_nearest_dev): the bit plane of (1), then a row and a column pass ------------------------------
// (2') the signed offset ex - x of the nearest edge pixel of the row within `radius`, the smaller ex (the left one) on a tie; kNoRowEdge when none
constexpr int kNoRowEdge = 127;                                    // radius <= 32: every offset fits an int8 beside it
__global__ __launch_bounds__(256) void edge_row_near_kernel(const unsigned long long *__restrict__ bits, uint32_t width, uint32_t height, uint32_t words_per_row,
                                                            uint32_t radius, int8_t *__restrict__ row_off)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    uint32_t dl, dr;
    row_edge_distances(bits + (size_t)y * words_per_row, x, words_per_row, dl, dr);
    const int off = dl <= dr ? -(int)dl : (int)dr;                  // (dl == dr == 0: the pixel itself)
    const uint32_t d = dl <= dr ? dl : dr;
    row_off[(size_t)y * width + x] = (int8_t)(d <= radius ? off : kNoRowEdge);
}

// (3') over the rows y - radius .. y + radius inside the frame, ascending, the candidate of least dx^2 + dy^2; the first one on a tie (the smaller
// ey; within a row (2') already took the smaller ex): the lexicographic minimum of (d^2, ey, ex) over the window, exactly
__global__ __launch_bounds__(256) void edge_col_near_kernel(const int8_t *__restrict__ row_off, uint32_t width, uint32_t height, uint32_t radius,
                                                            uint32_t *__restrict__ nearest)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const int y_lo = max((int)y - (int)radius, 0), y_hi = min((int)y + (int)radius, (int)height - 1);
    uint32_t best_d2 = 0xffffffffu, best = PR_EDGE_NONE;
    for (int yy = y_lo; yy <= y_hi; ++yy) {
        const int off = row_off[(size_t)yy * width + x];
        if (off == kNoRowEdge) continue;
        const int dy = yy - (int)y;
        const uint32_t d2 = (uint32_t)(off * off + dy * dy);
        if (d2 < best_d2) { best_d2 = d2; best = ((uint32_t)yy << 16) | (uint32_t)((int)x + off); }
    }
    nearest[(size_t)y * width + x] = best;
}

hipError_t launch_scene_edge_nearest(const void *scene, bool scene_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                                     unsigned long long *bits, int8_t *row_off, uint32_t *nearest, hipStream_t s)
{
    const uint32_t wpr = overlap_words_per_row(width), cells = height * wpr;
    with_scene(scene, scene_i32, [&](auto *sc) { hipLaunchKernelGGL(scene_edge_kernel, dim3((cells + 3) / 4), dim3(256), 0, s, sc, width, height, jump_mm, bits, wpr); });
    const dim3 grid((width + 255) / 256, height);
    hipLaunchKernelGGL(edge_row_near_kernel, grid, dim3(256), 0, s, bits, width, height, wpr, radius, row_off);
    hipLaunchKernelGGL(edge_col_near_kernel, grid, dim3(256), 0, s, row_off, width, height, radius, nearest);
    return hipGetLastError();
}

// ---- hypothesis side ----------------------------------------------------------------------------------------------------------------
// score_box_kernel's shape: one workgroup = 16 image rows of one hypothesis' box, 4 wavefronts x 4 rows, lanes along a row.  Per 64-column
// strip a wavefront loads its four rows and the row above and below once (six row loads for four output rows); the left and right
// neighbours come from the neighbouring lanes, and one more load per row, by lanes 0 and 63 only, fetches the two columns beside the strip.
// `win` {x0, row0, x1, row1} is the image the render lives in (the frame, or the ROI window) in image coordinates: a neighbour outside it
// is ignored, one inside it but outside the packed box is empty by construction.  Only contour pixels (a few per cent) read the scene
// and the distance image, which stay in L2 and are shared by every hypothesis.  Counts per lane in registers, summed over the workgroup
// (block_totals), one integer atomic per counter and workgroup: exact and independent of chunking and batch composition.
// dist_sum: a workgroup covers kBoxRowsPerBlock rows x <= kMaxFrameSide columns of D <= 255, so its sum stays below 2^25 -- 32 bits per lane
// and workgroup are enough (no low / high split as abs_err_sum needs), and only the per-hypothesis total needs the 64-bit atomic.
constexpr uint64_t kMaxFrameSide = 8192;                          // frame_size_ok (pr_runtime.h) refuses wider or taller frames
static_assert(kBoxRowsPerBlock * kMaxFrameSide * 255 < (1ull << 32), "contour_box_kernel: a workgroup's dist_sum must fit 32 bits");
template <typename SceneT>
__global__ __launch_bounds__(256) void contour_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                          const uint32_t *__restrict__ box_off, const int4 win, const SceneT *__restrict__ scene,
                                                          const uint8_t *__restrict__ edge_dist, int32_t tau, int32_t jump_mm, uint32_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63;
    BoxBlock blk;
    if (!box_block(bbox, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
    const int64_t t = tau, jump = jump_mm;
    // rows row0 - 1 .. row0 + 4: in the box (a line to load from), else inside the image (empty) or outside it (ignored) -- per wavefront
    const int32_t *line[6];
    int32_t off_box[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int row = row0 - 1 + k;
        const bool in_box = row >= r_lo && row <= r_hi;
        line[k] = in_box ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, (uint32_t)row, width, height) : depth;
        off_box[k] = in_box ? 1 : ((row >= win.y && row <= win.w) ? 0 : kNoNeighbour);
    }
    auto value = [](int32_t d) { return rendered(d) ? d : 0; };                         // nothing drawn -> empty
    uint32_t con = 0, hit = 0, occ = 0, mis = 0, dsum = 0;
    for (int x0 = bb.x; x0 <= bb.z; x0 += 64) {
        const int x = x0 + (int)lane;
        const bool in_x = x <= bb.z;
        const int xe = lane == 0 ? x0 - 1 : x0 + 64;                                    // the columns beside the strip: lanes 0 and 63
        const bool ends = lane == 0 || lane == 63;
        const int32_t side_out = (xe >= win.x && xe <= win.z) ? 0 : kNoNeighbour;
        const bool side_in = ends && xe >= bb.x && xe <= bb.z;
        int32_t v[6], e[4];                                          // 10 loads in flight per lane before the first compare
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = (off_box[k] == 1) ? (in_x ? value(line[k][x]) : ((x <= win.z) ? 0 : kNoNeighbour)) : off_box[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = (off_box[k + 1] == 1 && side_in) ? value(line[k + 1][xe]) : side_out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t c = v[k + 1];
            const int32_t up = __shfl_up(c, 1), dn = __shfl_down(c, 1);
            const int32_t l = lane == 0 ? e[k] : up, r = lane == 63 ? e[k] : dn;
            if (!(off_box[k + 1] == 1 && in_x && c > 0)) continue;
            if (!(edge_trigger(c, l, jump) || edge_trigger(c, r, jump) || edge_trigger(c, v[k], jump) || edge_trigger(c, v[k + 2], jump))) continue;
            const size_t px = (size_t)(row0 + k) * width + (size_t)x;
            const int32_t s = (int32_t)scene[px];
            const uint32_t D = edge_dist[px];
            ++con;
            if (depth_class(c, s, t) == 1) ++occ;                   // scene surface in front of the contour: no edge can be expected
            else if (D != 255) { ++hit; dsum += D; }
            else ++mis;
        }
    }
    const uint32_t cnt[5] = { con, hit, occ, mis, dsum };
    const uint32_t sum = block_totals(cnt), k = threadIdx.x;
    uint32_t *rec = records + (size_t)blockIdx.y * 8;
    if (sum && k < 4) atomicAdd(rec + k, sum);
    else if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), (unsigned long long)sum);      // (k == 4: the others' totals are 0)
}

hipError_t launch_contour_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                                const void *scene, bool scene_i32, const uint8_t *edge_dist, int32_t tau, int32_t jump_mm, uint32_t *records, hipStream_t s)
{
    return for_box_launches(depth, box_off, n_poses, width, height, scene, scene_i32, [&](const BoxLaunch &b, auto *sc) {
        hipLaunchKernelGGL(contour_box_kernel, b.grid, dim3(256), 0, s, b.depth, bbox + b.p0, width, height, b.box_off, window, sc, edge_dist, tau, jump_mm,
                           records + (size_t)b.p0 * 8);
    });
}

}  // namespace prk
