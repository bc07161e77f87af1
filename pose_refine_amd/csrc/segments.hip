// segments.hip -- the depth-connected components of a frame (pr_scene_segments_dev; the definition is in include/pose_refine.h, its one
// implementation in segments.h): a union-find forest over the pixels whose every link points to a LOWER pixel index, so a component's root is
// its lowest pixel whatever the order of arrival.  Tiles are solved in LDS, the links across tile borders are united by atomicMin on the global
// forest, one pass flattens it and counts, the qualifying roots are compacted in root order (count, scan, emit), and -- once the host has
// ordered them -- one pass writes the labels and accumulates the records.  Integers only.  No kernel waits for another workgroup: every loop
// walks a strictly decreasing chain of pixel indices or clears at least one bit of a lane mask per turn.
// gfx950 (CDNA4, wave64).
#include "pr_launch.h"
#include "segments.h"

namespace prk {

using segments::kNone;

constexpr uint32_t kSegTileW = 64, kSegTileH = 16;               // a tile: a wavefront per row, 16 rows (compose.hip's tile)
constexpr uint32_t kSegBlock = 1024;                             // the flatten pass: 1024 pixel indices per workgroup
constexpr uint32_t kSegThreads = 256;

// ---- the forest: parent[x] <= x always; a word is only ever lowered ------------------------------------------------------------------------
// Words of the forest that another lane may lower while they are read are read by atomic loads and lowered by atomicMin alone: in LDS at
// workgroup scope (the tile pass), in memory at agent scope (the seam pass: L1 is per CU, the L2s per XCD -- a plain load could stay stale for
// the whole launch; an agent-scope load is served past both).  A stale find is harmless in exactly this union: the value atomicMin RETURNS
// decides, and whatever it displaced is united in turn.
struct LdsWords {
    static __device__ __forceinline__ uint32_t load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ uint32_t lower(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct AgentWords {
    static __device__ __forceinline__ uint32_t load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t lower(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// the root above x: the chain falls strictly, so it ends after at most x steps (a word that is not below its index ends it)
template <class Words>
__device__ __forceinline__ uint32_t forest_find(uint32_t *parent, uint32_t x)
{
    for (uint32_t p; (p = Words::load(parent + x)) < x; ) x = p;
    return x;
}
// unite the components of a and b: the higher root is lowered to the other; when it was no root any more, go on with what it pointed to.
// a + b falls with every turn that does not end the loop.
template <class Words>
__device__ __forceinline__ void forest_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = forest_find<Words>(parent, a);
        b = forest_find<Words>(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = Words::lower(parent + a, b);
        if (old >= a) return;                                      // a was a root (old == a) and now hangs under b
        a = old;
    }
}

__global__ __launch_bounds__(kSegThreads) void segment_init_kernel(SegControl *__restrict__ ctl, segments::Acc *__restrict__ acc, uint32_t n_acc)
{
    const uint32_t t = blockIdx.x * kSegThreads + threadIdx.x;
    if (t == 0) *ctl = SegControl{ 0u, 0u, { 0u, 0u } };
    if (t < n_acc) acc[t] = segments::acc_empty();
}

// ---- tiles: a workgroup per 64 x 16 tile, a wavefront per row ------------------------------------------------------------------------------
// Horizontal runs: one ballot of "starts a run" (measured and not linked to its left neighbour); a lane's run starts at the highest such bit at
// or below it.  Vertical links are united in LDS, one per contact: a link whose left neighbours are linked the same way (left, up-left and
// both horizontal links) adds nothing and is skipped.  Then every pixel takes its tile-local root as a global pixel index.
template <class T>
__global__ __launch_bounds__(kSegTileW * kSegTileH) void segment_tile_kernel(const T *__restrict__ depth, uint32_t width, uint32_t height, uint32_t jump,
                                                                             uint32_t *__restrict__ parent, uint32_t *__restrict__ count)
{
    __shared__ uint32_t s_d[kSegTileW * kSegTileH], s_p[kSegTileW * kSegTileH];
    const uint32_t lane = threadIdx.x, row = threadIdx.y, t = row * kSegTileW + lane;
    const uint32_t x = blockIdx.x * kSegTileW + lane, y = blockIdx.y * kSegTileH + row;
    const bool inside = x < width && y < height;
    const size_t i = (size_t)y * width + x;
    const uint32_t d = inside ? segments::depth_of(depth[i]) : 0u;
    s_d[t] = d;
    const uint32_t d_left = (uint32_t)__shfl_up((int)d, 1);
    const bool link_left = lane > 0 && segments::linked(d, d_left, jump);
    const unsigned long long starts = __ballot(d != 0u && !link_left);
    const unsigned long long below = starts & (~0ull >> (63u - lane));
    s_p[t] = (d != 0u && below) ? row * kSegTileW + (63u - (uint32_t)__clzll(below)) : kNone;
    __syncthreads();
    if (row > 0 && d != 0u) {
        const uint32_t d_up = s_d[t - kSegTileW];
        if (segments::linked(d, d_up, jump)) {
            bool redundant = false;
            if (link_left) { const uint32_t d_ul = s_d[t - kSegTileW - 1]; redundant = segments::linked(d_left, d_ul, jump) && segments::linked(d_up, d_ul, jump); }
            if (!redundant) forest_union<LdsWords>(s_p, t, t - kSegTileW);
        }
    }
    __syncthreads();
    if (!inside) return;
    count[i] = 0;
    uint32_t root = kNone;
    if (d != 0u) {
        const uint32_t r = forest_find<LdsWords>(s_p, t);
        root = (blockIdx.y * kSegTileH + r / kSegTileW) * width + blockIdx.x * kSegTileW + r % kSegTileW;
    }
    parent[i] = root;
}

// ---- seams: a thread per pixel pair across a tile border ---------------------------------------------------------------------------------
// First the pairs across the vertical borders (x = 64 c, its left neighbour), all of them; then those across the horizontal borders (y = 16 r,
// the pixel above), skipped by the tile pass' rule.  (Only the second kind skips: a skipped link relies on horizontal links and on the link one
// column to the left, which ends at a column that does not skip.)
template <class T>
__global__ __launch_bounds__(kSegThreads) void segment_seam_kernel(const T *__restrict__ depth, uint32_t width, uint32_t height, uint32_t jump, uint32_t n_vertical,
                                                                   uint32_t n_total, uint32_t *parent)
{
    const uint32_t t = blockIdx.x * kSegThreads + threadIdx.x;
    if (t >= n_total) return;
    if (t < n_vertical) {
        const uint32_t x = (t / height + 1u) * kSegTileW, y = t % height;
        const size_t i = (size_t)y * width + x;
        if (segments::linked(segments::depth_of(depth[i]), segments::depth_of(depth[i - 1]), jump)) forest_union<AgentWords>(parent, (uint32_t)i, (uint32_t)i - 1u);
        return;
    }
    const uint32_t u = t - n_vertical, x = u % width, y = (u / width + 1u) * kSegTileH;
    const size_t i = (size_t)y * width + x;
    const uint32_t d = segments::depth_of(depth[i]), d_up = segments::depth_of(depth[i - width]);
    if (!segments::linked(d, d_up, jump)) return;
    if (x > 0) {
        const uint32_t d_left = segments::depth_of(depth[i - 1]), d_ul = segments::depth_of(depth[i - width - 1]);
        if (segments::linked(d, d_left, jump) && segments::linked(d_left, d_ul, jump) && segments::linked(d_up, d_ul, jump)) return;
    }
    forest_union<AgentWords>(parent, (uint32_t)i, (uint32_t)i - width);
}

// ---- reductions over a wavefront (every lane takes part: a lane outside a group brings the identity) ------------------------------------------------
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { for (int off = 32; off; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, off); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { for (int off = 32; off; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, off); v = o > v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) { for (int off = 32; off; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off); return v; }
__device__ __forceinline__ unsigned long long wave_add_u64(unsigned long long v) { for (int off = 32; off; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off); return v; }

// ---- flatten and count: every pixel takes its root; a workgroup adds to count[root] once per distinct root among its wavefronts' first roots ----
// (a launch of its own: the forest is final.  Lanes store roots into words that others walk through -- every value ever stored there is an
// ancestor in the final forest, so a walk ends at the same root whichever it meets.)  A wavefront counts its lanes per distinct root; the count of
// its FIRST root goes through LDS, where the first wavefront adds up the wavefronts that share a root -- a large component then costs one global
// atomic per 1024 pixels, not one per 64 -- and those of its further roots go straight to memory.
__global__ __launch_bounds__(kSegBlock) void segment_flatten_kernel(uint32_t n_px, uint32_t *parent, uint32_t *__restrict__ count)
{
    __shared__ uint32_t s_root[kSegBlock / 64], s_n[kSegBlock / 64];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t r = kNone;
    if (i < n_px && parent[i] != kNone) {
        r = forest_find<AgentWords>(parent, i);
        parent[i] = r;
    }
    unsigned long long todo = __ballot(r != kNone);
    if (lane == 0) { s_root[wave] = kNone; s_n[wave] = 0; }
    bool first = true;
    while (todo) {                                                 // one turn per distinct root of the wavefront
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t k = (uint32_t)__shfl((int)r, (int)leader);
        const unsigned long long group = __ballot(r == k);
        if (lane == leader) {
            if (first) { s_root[wave] = k; s_n[wave] = (uint32_t)__popcll(group); }
            else atomicAdd(&count[k], (uint32_t)__popcll(group));
        }
        first = false;
        todo &= ~group;
    }
    __syncthreads();
    if (wave != 0) return;
    const uint32_t wr = lane < kSegBlock / 64 ? s_root[lane] : kNone, wn = lane < kSegBlock / 64 ? s_n[lane] : 0u;
    todo = __ballot(wr != kNone);
    while (todo) {                                                 // one turn per distinct first root of the workgroup
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t k = (uint32_t)__shfl((int)wr, (int)leader);
        const bool mine = wr == k;
        const uint32_t n = wave_add_u32(mine ? wn : 0u);
        if (lane == leader) atomicAdd(&count[k], n);
        todo &= ~__ballot(mine);
    }
}

// ---- the qualifying roots in root order: a wavefront per chunk of kSegChunk pixel indices (count, scan, emit) --------------------------------
__global__ __launch_bounds__(64) void segment_root_count_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ count, uint32_t n_px, uint32_t min_pixels,
                                                                uint32_t *__restrict__ chunk_count, SegControl *__restrict__ ctl)
{
    const uint32_t first = blockIdx.x * kSegChunk;
    uint32_t n_roots = 0;                                          // this lane's roots, qualifying or not: the keep test meets them all
    const uint32_t n_keep = wave_compact_count(kSegChunk, threadIdx.x, [&](uint32_t o) {
        const uint32_t i = first + o;
        const bool is_root = i < n_px && parent[i] == i;
        n_roots += is_root ? 1u : 0u;
        return is_root && count[i] >= min_pixels;
    });
    n_roots = wave_sum_u32(n_roots);
    if (threadIdx.x == 0) {
        chunk_count[blockIdx.x] = n_keep;
        if (n_roots) atomicAdd(&ctl->n_components, n_roots);
    }
}
// count[root] becomes the root's position in the list (kNone: it does not qualify, or the list is full -- the call fails then).  On
// wave_compact_step, not wave_compact_place: a root that is not kept is rewritten as well, and the test and the stores share one load of
// parent[i] and count[i], which a keep test and a visitor apart would each make.
__global__ __launch_bounds__(64) void segment_root_emit_kernel(const uint32_t *__restrict__ parent, uint32_t *__restrict__ count, uint32_t n_px, uint32_t min_pixels,
                                                               const uint32_t *__restrict__ chunk_off, SegRoot *__restrict__ roots)
{
    const uint32_t first = blockIdx.x * kSegChunk;
    uint32_t base = chunk_off[blockIdx.x];
    for (uint32_t o0 = 0; o0 < kSegChunk; o0 += 64) {
        const uint32_t i = first + o0 + threadIdx.x;
        const bool is_root = i < n_px && parent[i] == i;
        const uint32_t pixels = is_root ? count[i] : 0u;
        const bool keep = is_root && pixels >= min_pixels;
        const WaveSlot slot = wave_compact_step(keep, threadIdx.x, base);
        const bool stored = keep && slot.pos < PR_SEGMENT_MAX_ROOTS;
        if (stored) roots[slot.pos] = SegRoot{ i, pixels };
        if (is_root) count[i] = stored ? slot.pos : kNone;
        base += slot.kept;
    }
}
// the control words and the stored roots into the pinned block, by a grid that does not depend on how many there are
__global__ __launch_bounds__(kSegThreads) void segment_export_kernel(const SegControl *__restrict__ ctl, const SegRoot *__restrict__ roots, uint32_t *__restrict__ out)
{
    const uint32_t t = blockIdx.x * kSegThreads + threadIdx.x;
    const uint32_t nq = ctl->n_qualifying, n_words = 2u * (nq < PR_SEGMENT_MAX_ROOTS ? nq : (uint32_t)PR_SEGMENT_MAX_ROOTS);
    if (t < 4) out[t] = reinterpret_cast<const uint32_t *>(ctl)[t];
    if (t < n_words) out[4 + t] = reinterpret_cast<const uint32_t *>(roots)[t];
}

// ---- labels and records ----------------------------------------------------------------------------------------------------------------
struct AtomicOp {
    __device__ __forceinline__ void min32(uint32_t *p, uint32_t v) const { atomicMin(p, v); }
    __device__ __forceinline__ void max32(uint32_t *p, uint32_t v) const { atomicMax(p, v); }
    __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) const { atomicAdd(p, v); }
    __device__ __forceinline__ void add64(uint64_t *p, uint64_t v) const { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }
};
// A wavefront is 64 pixels of one row, a workgroup a 64 x 16 tile.  The lanes of one label are reduced together (the box from the lane mask, the
// depth range and the sums by shuffles) into one piece.  The piece of a wavefront's FIRST label goes through LDS, where the first wavefront
// merges the pieces of equal label the same way and one lane merges the result into the label's record: ten atomics per label and tile for a
// large segment, not per pixel and not per row.  Pieces of a wavefront's further labels (a row of small blobs) go straight to the record.
__device__ __forceinline__ segments::Part reduce_part(bool mine, const segments::Part &q)
{
    segments::Part p;
    p.x0 = wave_min_u32(mine ? q.x0 : kNone); p.y0 = wave_min_u32(mine ? q.y0 : kNone); p.dmin = wave_min_u32(mine ? q.dmin : kNone);
    p.x1 = wave_max_u32(mine ? q.x1 : 0u); p.y1 = wave_max_u32(mine ? q.y1 : 0u); p.dmax = wave_max_u32(mine ? q.dmax : 0u);
    p.n = wave_add_u32(mine ? q.n : 0u);
    p.sx = wave_add_u64(mine ? q.sx : 0ull); p.sy = wave_add_u64(mine ? q.sy : 0ull); p.sd = wave_add_u64(mine ? q.sd : 0ull);
    return p;
}
template <class T>
__global__ __launch_bounds__(kSegTileW * kSegTileH) void segment_relabel_kernel(const T *__restrict__ depth, uint32_t width, uint32_t height, const uint32_t *__restrict__ parent,
                                                                                const uint32_t *__restrict__ slot, const uint16_t *__restrict__ rank_label, uint32_t n_found,
                                                                                uint16_t *__restrict__ labels, uint32_t *__restrict__ roots_out, segments::Acc *acc)
{
    __shared__ segments::Part s_part[kSegTileH];
    __shared__ uint32_t s_key[kSegTileH];
    const uint32_t lane = threadIdx.x, wave = threadIdx.y, x = blockIdx.x * kSegTileW + lane, y = blockIdx.y * kSegTileH + wave;
    uint32_t lab = 0, d = 0;
    if (x < width && y < height) {
        const size_t i = (size_t)y * width + x;
        const uint32_t r = parent[i];
        if (roots_out) roots_out[i] = r;
        if (r != kNone) {
            const uint32_t sl = slot[r];
            lab = sl == kNone ? (uint32_t)PR_SEGMENT_DROPPED : (uint32_t)rank_label[sl];
            d = segments::depth_of(depth[i]);
        }
        labels[i] = (uint16_t)lab;
    }
    const uint32_t key = (lab >= 1u && lab <= n_found) ? lab : 0u;
    const segments::Part own = segments::part_of_pixel(x, y, d);
    unsigned long long todo = __ballot(key != 0u);
    if (lane == 0) s_key[wave] = 0;
    bool first = true;
    while (todo) {                                                 // one turn per distinct label of the wavefront
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t k = (uint32_t)__shfl((int)key, (int)leader);
        const bool mine = key == k;
        const segments::Part p = reduce_part(mine, own);
        if (lane == leader) {
            if (first) { s_part[wave] = p; s_key[wave] = k; }
            else segments::acc_merge(&acc[k - 1u], p, AtomicOp{});
        }
        first = false;
        todo &= ~__ballot(mine);
    }
    __syncthreads();
    if (wave != 0) return;
    const uint32_t wkey = lane < kSegTileH ? s_key[lane] : 0u;
    const segments::Part wpart = s_part[lane < kSegTileH ? lane : 0u];       // (read only where wkey != 0: the wavefront stored it)
    todo = __ballot(wkey != 0u);
    while (todo) {                                                 // one turn per distinct first label of the tile
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t k = (uint32_t)__shfl((int)wkey, (int)leader);
        const bool mine = wkey == k;
        const segments::Part p = reduce_part(mine, wpart);
        if (lane == leader) segments::acc_merge(&acc[k - 1u], p, AtomicOp{});
        todo &= ~__ballot(mine);
    }
}

template <class T>
__global__ __launch_bounds__(kSegThreads) void segment_depth_kernel(const uint16_t *__restrict__ labels, const T *depth_in, T *depth_out, uint32_t n_px,
                                                                    const uint32_t *__restrict__ keep_bits, uint32_t n_keep)
{
    const uint32_t i = blockIdx.x * kSegThreads + threadIdx.x;     // (depth_out may be depth_in: a thread reads and writes its own pixel only)
    if (i >= n_px) return;
    const uint32_t lab = labels[i];
    const bool keep = lab < n_keep && ((keep_bits[lab >> 5] >> (lab & 31u)) & 1u);
    depth_out[i] = keep ? depth_in[i] : (T)0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
hipError_t launch_segment_init(SegControl *ctl, segments::Acc *acc, uint32_t n_acc, hipStream_t s)
{
    hipLaunchKernelGGL(segment_init_kernel, dim3(n_acc / kSegThreads + 1), dim3(kSegThreads), 0, s, ctl, acc, n_acc);
    return hipGetLastError();
}

hipError_t launch_segment_tiles(const void *depth, bool depth_i32, uint32_t width, uint32_t height, uint32_t jump, uint32_t *parent, uint32_t *count, hipStream_t s)
{
    const dim3 grid((width + kSegTileW - 1) / kSegTileW, (height + kSegTileH - 1) / kSegTileH), block(kSegTileW, kSegTileH);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(segment_tile_kernel<T>, grid, block, 0, s, static_cast<const T *>(depth), width, height, jump, parent, count);
    });
    return hipGetLastError();
}

hipError_t launch_segment_seams(const void *depth, bool depth_i32, uint32_t width, uint32_t height, uint32_t jump, uint32_t *parent, hipStream_t s)
{
    const uint32_t n_vertical = ((width + kSegTileW - 1) / kSegTileW - 1) * height, n_total = n_vertical + ((height + kSegTileH - 1) / kSegTileH - 1) * width;
    if (n_total == 0) return hipSuccess;                           // one tile: no seam (the frame's size decides, not its content)
    const dim3 grid((n_total + kSegThreads - 1) / kSegThreads);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(segment_seam_kernel<T>, grid, dim3(kSegThreads), 0, s, static_cast<const T *>(depth), width, height, jump, n_vertical, n_total, parent);
    });
    return hipGetLastError();
}

hipError_t launch_segment_flatten(uint32_t width, uint32_t height, uint32_t *parent, uint32_t *count, hipStream_t s)
{
    const uint32_t n_px = width * height;
    hipLaunchKernelGGL(segment_flatten_kernel, dim3((n_px + kSegBlock - 1) / kSegBlock), dim3(kSegBlock), 0, s, n_px, parent, count);
    return hipGetLastError();
}

hipError_t launch_segment_compact(const uint32_t *parent, uint32_t *count, uint32_t n_px, uint32_t min_pixels, uint32_t *chunk_count, uint32_t *chunk_off,
                                  SegRoot *roots, SegControl *ctl, void *out_mapped, hipStream_t s)
{
    const uint32_t n_chunks = (n_px + kSegChunk - 1) / kSegChunk;
    hipLaunchKernelGGL(segment_root_count_kernel, dim3(n_chunks), dim3(64), 0, s, parent, (const uint32_t *)count, n_px, min_pixels, chunk_count, ctl);
    { hipError_t e = launch_scan_counts(chunk_count, n_chunks, chunk_off, &ctl->n_qualifying, false, s); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(segment_root_emit_kernel, dim3(n_chunks), dim3(64), 0, s, parent, count, n_px, min_pixels, (const uint32_t *)chunk_off, roots);
    hipLaunchKernelGGL(segment_export_kernel, dim3(2 * PR_SEGMENT_MAX_ROOTS / kSegThreads), dim3(kSegThreads), 0, s, (const SegControl *)ctl, (const SegRoot *)roots,
                       static_cast<uint32_t *>(out_mapped));
    return hipGetLastError();
}

hipError_t launch_segment_relabel(const void *depth, bool depth_i32, uint32_t width, uint32_t height, const uint32_t *parent, const uint32_t *slot,
                                  const uint16_t *rank_label, uint32_t n_found, uint16_t *labels, uint32_t *roots_out, segments::Acc *acc, hipStream_t s)
{
    const dim3 grid((width + kSegTileW - 1) / kSegTileW, (height + kSegTileH - 1) / kSegTileH), block(kSegTileW, kSegTileH);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(segment_relabel_kernel<T>, grid, block, 0, s, static_cast<const T *>(depth), width, height, parent, slot, rank_label, n_found, labels, roots_out, acc);
    });
    return hipGetLastError();
}

hipError_t launch_segment_depth(const uint16_t *labels, const void *depth_in, void *depth_out, bool depth_i32, uint32_t n_px, const uint32_t *keep_bits,
                                uint32_t n_keep, hipStream_t s)
{
    const dim3 grid((n_px + kSegThreads - 1) / kSegThreads);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(segment_depth_kernel<T>, grid, dim3(kSegThreads), 0, s, labels, static_cast<const T *>(depth_in), static_cast<T *>(depth_out), n_px, keep_bits, n_keep);
    });
    return hipGetLastError();
}

}  // namespace prk
