// depth_filter.hip -- depth conditioning of a frame (pr_depth_filter_dev, pr_depth_fuse_dev; the definition is in include/pose_refine.h, its one
// implementation in depth_filter.h).  The filter is one stencil launch: a workgroup per 64 x 16 tile, one pixel per lane; the gated tile and a
// halo of three pixels go into LDS, the flying test turns them into F for the tile and a halo of two, and every lane selects the lower median
// of its window in registers.  The fuse is element-wise: a lane per pixel, or per 16 bytes of pixels where every pointer allows it.  Integers
// only, no float anywhere.  No kernel waits for another workgroup and no loop's trip count depends on data.
// gfx950 (CDNA4, wave64).
#include "pr_launch.h"
#include "depth_filter.h"

namespace prk {

constexpr uint32_t kDfTileW = 64, kDfTileH = 16;                 // a tile: a wavefront per row, 16 rows (segments.hip's tile)
constexpr uint32_t kDfHaloG = PR_DEPTH_FILTER_MAX_RADIUS + 1, kDfHaloF = PR_DEPTH_FILTER_MAX_RADIUS;      // the flying test looks one pixel beyond the window
constexpr uint32_t kDfGW = kDfTileW + 2 * kDfHaloG, kDfGH = kDfTileH + 2 * kDfHaloG;       // 70 x 22 words of G
constexpr uint32_t kDfFW = kDfTileW + 2 * kDfHaloF, kDfFH = kDfTileH + 2 * kDfHaloF;       // 68 x 20 words of F
constexpr uint32_t kDfThreads = kDfTileW * kDfTileH;
constexpr uint32_t kFuseThreads = 256;

__global__ __launch_bounds__(64) void depth_filter_init_kernel(FilterControl *__restrict__ ctl)
{
    if (threadIdx.x < sizeof(FilterControl) / sizeof(uint32_t)) reinterpret_cast<uint32_t *>(ctl)[threadIdx.x] = 0u;
}

// ---- the filter: a workgroup per tile --------------------------------------------------------------------------------------------------------
// s_g: G on the tile and three pixels around it (0 outside the frame).  s_f: F on the tile and two pixels around it, each from the 3 x 3 of
// s_g around it.  A lane's window is (2 R + 1)^2 words of s_f at compile-time offsets from its own.  The rows are 70 and 68 words: the lanes of
// a wavefront read consecutive words, whatever the offset.
template <class T, int R>
__global__ __launch_bounds__(kDfThreads) void depth_filter_kernel(const T *__restrict__ depth_in, uint32_t width, uint32_t height, pr_depth_filter_params prm,
                                                                  T *__restrict__ depth_out, uint8_t *__restrict__ flags, FilterControl *ctl)
{
    __shared__ uint32_t s_g[kDfGW * kDfGH], s_f[kDfFW * kDfFH], s_n[6];
    const uint32_t lane = threadIdx.x, row = threadIdx.y, t = row * kDfTileW + lane;
    const int ox = (int)(blockIdx.x * kDfTileW), oy = (int)(blockIdx.y * kDfTileH);
    if (t < 6) s_n[t] = 0u;
    for (uint32_t c = t; c < kDfGW * kDfGH; c += kDfThreads) {
        const int x = ox + (int)(c % kDfGW) - (int)kDfHaloG, y = oy + (int)(c / kDfGW) - (int)kDfHaloG;
        uint32_t g = 0u;
        if (x >= 0 && y >= 0 && x < (int)width && y < (int)height) g = dfilt::gate(dfilt::depth_of(depth_in[(size_t)y * width + (size_t)x]), prm);
        s_g[c] = g;
    }
    __syncthreads();
    for (uint32_t c = t; c < kDfFW * kDfFH; c += kDfThreads) {
        const uint32_t at = (c / kDfFW + 1u) * kDfGW + c % kDfFW + 1u;       // the same pixel in s_g: one halo pixel further in
        s_f[c] = dfilt::flying(prm, [&](int dx, int dy) { return s_g[(int)at + dy * (int)kDfGW + dx]; });
    }
    __syncthreads();
    const uint32_t x = (uint32_t)ox + lane, y = (uint32_t)oy + row;
    const bool inside = x < width && y < height;
    uint32_t flag = 0xFFu;                                         // a lane outside the frame counts for no code
    if (inside) {
        const size_t i = (size_t)y * width + x;
        const uint32_t d0 = dfilt::depth_of(depth_in[i]);
        const uint32_t fat = (row + kDfHaloF) * kDfFW + lane + kDfHaloF;
        const dfilt::Out o = dfilt::pixel_out<R>(prm, d0, s_g[(row + kDfHaloG) * kDfGW + lane + kDfHaloG],
                                                 [&](int dx, int dy) { return s_f[(int)fat + dy * (int)kDfFW + dx]; });
        depth_out[i] = (T)o.depth;
        if (flags) flags[i] = (uint8_t)o.flag;
        flag = o.flag;
    }
    // the counts: a wavefront's lanes per code by ballot, the wavefronts' in LDS, one atomic per code the tile has
#pragma unroll
    for (uint32_t c = 0; c < 6; ++c) {
        const uint32_t n = (uint32_t)__popcll(__ballot(flag == c));
        if (lane == 0 && n) atomicAdd(&s_n[c], n);
    }
    __syncthreads();
    if (t < 6 && s_n[t]) atomicAdd(&ctl->n[t], s_n[t]);
}

// ---- the fuse: element-wise over up to eight frames -----------------------------------------------------------------------------------------
// (depth_out may be one of the frames: no __restrict__ on either, and a lane has read every value of its pixels before it stores)
// VEC: 16 bytes of pixels per lane -- eight uint16 or four int32 -- over the first n_px / PER groups, then a lane per pixel of the tail
template <class T, bool VEC>
__global__ __launch_bounds__(kFuseThreads) void depth_fuse_kernel(FuseFrames frames, uint32_t n_frames, uint32_t n_px, uint32_t min_frames, T *depth_out, uint8_t *count_out)
{
    constexpr uint32_t PER = 16u / sizeof(T);
    const uint32_t t = blockIdx.x * kFuseThreads + threadIdx.x;
    const uint32_t n_groups = VEC ? n_px / PER : 0u, first_tail = n_groups * PER;
    if (VEC && t < n_groups) {
        union Pack { uint4 q; T e[PER]; };
        Pack in[kDepthFuseMax], out;
#pragma unroll
        for (uint32_t f = 0; f < kDepthFuseMax; ++f)
            if (f < n_frames) in[f].q = reinterpret_cast<const uint4 *>(frames.p[f])[t]; else in[f].q = make_uint4(0u, 0u, 0u, 0u);
        union Counts { uint2 w; uint8_t b[8]; } cnt;
        cnt.w = make_uint2(0u, 0u);
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            uint32_t v[8], k;
#pragma unroll
            for (uint32_t f = 0; f < kDepthFuseMax; ++f) v[f] = dfilt::depth_of(in[f].e[e]);
            out.e[e] = (T)dfilt::fuse(v, min_frames, &k);
            cnt.b[e] = (uint8_t)k;
        }
        reinterpret_cast<uint4 *>(depth_out)[t] = out.q;
        if (count_out) {
            if (PER == 8) reinterpret_cast<uint2 *>(count_out)[t] = cnt.w; else reinterpret_cast<uint32_t *>(count_out)[t] = cnt.w.x;
        }
        return;
    }
    const uint32_t i = first_tail + (t - n_groups);
    if (i >= n_px) return;
    uint32_t v[8], k;
#pragma unroll
    for (uint32_t f = 0; f < kDepthFuseMax; ++f) v[f] = f < n_frames ? dfilt::depth_of(static_cast<const T *>(frames.p[f])[i]) : 0u;
    depth_out[i] = (T)dfilt::fuse(v, min_frames, &k);
    if (count_out) count_out[i] = (uint8_t)k;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
hipError_t launch_depth_filter_init(FilterControl *ctl, hipStream_t s)
{
    hipLaunchKernelGGL(depth_filter_init_kernel, dim3(1), dim3(64), 0, s, ctl);
    return hipGetLastError();
}

hipError_t launch_depth_filter(const void *depth_in, bool depth_i32, uint32_t width, uint32_t height, const pr_depth_filter_params &params, void *depth_out,
                               uint8_t *flags, FilterControl *ctl, hipStream_t s)
{
    const dim3 grid((width + kDfTileW - 1) / kDfTileW, (height + kDfTileH - 1) / kDfTileH), block(kDfTileW, kDfTileH);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        const T *in = static_cast<const T *>(depth_in);
        T *out = static_cast<T *>(depth_out);
        if (params.radius == 0) hipLaunchKernelGGL((depth_filter_kernel<T, 0>), grid, block, 0, s, in, width, height, params, out, flags, ctl);
        else if (params.radius == 1) hipLaunchKernelGGL((depth_filter_kernel<T, 1>), grid, block, 0, s, in, width, height, params, out, flags, ctl);
        else hipLaunchKernelGGL((depth_filter_kernel<T, 2>), grid, block, 0, s, in, width, height, params, out, flags, ctl);
    });
    return hipGetLastError();
}

hipError_t launch_depth_fuse(const FuseFrames &frames, uint32_t n_frames, bool depth_i32, uint32_t n_px, uint32_t min_frames, void *depth_out, uint8_t *count_out,
                             hipStream_t s)
{
    // 16 bytes per lane where every pointer is on 16 bytes (the counts of a lane's pixels are 8 or 4 bytes: the same bound serves)
    uintptr_t bits = reinterpret_cast<uintptr_t>(depth_out) | reinterpret_cast<uintptr_t>(count_out);
    for (uint32_t f = 0; f < n_frames; ++f) bits |= reinterpret_cast<uintptr_t>(frames.p[f]);
    const bool vec = (bits & 15u) == 0;
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        const uint32_t per = 16u / (uint32_t)sizeof(T), n_threads = vec ? n_px / per + n_px % per : n_px;
        const dim3 grid((n_threads + kFuseThreads - 1) / kFuseThreads);
        if (vec) hipLaunchKernelGGL((depth_fuse_kernel<T, true>), grid, dim3(kFuseThreads), 0, s, frames, n_frames, n_px, min_frames, static_cast<T *>(depth_out), count_out);
        else hipLaunchKernelGGL((depth_fuse_kernel<T, false>), grid, dim3(kFuseThreads), 0, s, frames, n_frames, n_px, min_frames, static_cast<T *>(depth_out), count_out);
    });
    return hipGetLastError();
}

}  // namespace prk
