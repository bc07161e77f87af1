// reproject.hip -- z-buffered point reprojection (pr_depth_reproject_dev; the definition is in include/pose_refine.h, its one implementation in
// reproject.h).  Three launches.  Clear: the key plane to 0xFFFFFFFF, the control words to 0.  Scatter: the grid is cut into chunks by source; a lane
// reads 16 bytes of a frame (or four points of a cloud as three 16-byte loads), the workgroup turns them round in LDS so that the 64 lanes of a
// wavefront work on 64 consecutive pixels (points), and every sample writes its square with an integer atomicMin whose result is not used.
// Resolve: a workgroup per 64 x 16 tile with Z of the tile and a halo of two in LDS; the visibility test, the output, the source image and the
// counts; the tile that finishes last copies the control words into pinned memory.  No kernel waits for another workgroup.
// gfx950 (CDNA4, wave64).
#include "pr_launch.h"
#include "depth_filter.h"
#include "reproject.h"

namespace prk {

constexpr uint32_t kRpTileW = 64, kRpTileH = 16, kRpHalo = PR_REPROJECT_MAX_RADIUS;      // a tile: a wavefront per row, 16 rows (depth_filter.hip's tile)
constexpr uint32_t kRpZW = kRpTileW + 2 * kRpHalo, kRpZH = kRpTileH + 2 * kRpHalo;      // 68 x 20 words of Z
constexpr uint32_t kRpTileThreads = kRpTileW * kRpTileH;
constexpr uint32_t kRpControlWords = sizeof(ReprojControl) / sizeof(uint32_t);
constexpr uint32_t kRpWonWord = offsetof(ReprojControl, won) / sizeof(uint32_t);
static_assert(offsetof(ReprojControl, kept) == offsetof(ReprojControl, won) + 10 * sizeof(uint32_t), "ReprojControl: won[8], covered, hidden, kept in a row");
constexpr uint32_t kRpCloudPer = 4;                              // points per lane: 48 bytes

// ---- clear ---------------------------------------------------------------------------------------------------------------------------------
// (keys is the start of a device allocation: on 16 bytes)
__global__ __launch_bounds__(kReprojThreads) void reproject_clear_kernel(uint32_t *__restrict__ keys, uint32_t n_px, ReprojControl *__restrict__ ctl)
{
    const uint32_t t = blockIdx.x * kReprojThreads + threadIdx.x, n4 = n_px / 4u;
    if (t < n4) reinterpret_cast<uint4 *>(keys)[t] = make_uint4(rpj::kNoKey, rpj::kNoKey, rpj::kNoKey, rpj::kNoKey);
    else if (t - n4 < n_px % 4u) keys[n4 * 4u + (t - n4)] = rpj::kNoKey;
    if (blockIdx.x == 0 && threadIdx.x < kRpControlWords) reinterpret_cast<uint32_t *>(ctl)[threadIdx.x] = 0u;
}

// ---- scatter -------------------------------------------------------------------------------------------------------------------------------
// one sample: its outcome counted in n (samples, invalid, range, outside), its square written
__device__ __forceinline__ void scatter_sample(const rpj::Rigid &T, const rpj::Target &tg, uint32_t source, float px, float py, float pz, uint32_t *__restrict__ keys,
                                               uint32_t (&n)[4])
{
    const rpj::Splat sp = rpj::project(T, tg, px, py, pz);
    n[0] += 1u;
    n[1] += sp.code == rpj::kInvalid ? 1u : 0u;
    n[2] += sp.code == rpj::kRange ? 1u : 0u;
    n[3] += sp.code == rpj::kOutside ? 1u : 0u;
    if (sp.code != rpj::kDrawn) return;
    const uint32_t key = rpj::key_of(sp.d, source);
    for (int y = sp.y0; y < sp.y1; ++y)                            // (inside the frame: project() clipped the square)
        for (int x = sp.x0; x < sp.x1; ++x) atomicMin(&keys[(size_t)y * tg.width + (size_t)x], key);
}

// A frame source is one run of n elements; the slots of 16 bytes are cut on 16-byte ADDRESSES, so only the first and the last slot of a
// source can be partial, whatever the pointer and the row length.  A workgroup takes 256 slots: lane t loads slot t (one 16-byte load, or
// element by element for a partial slot, 0 where the source has no element) into LDS; then lane t works on elements t, 256 + t, ...
template <class D>
__device__ __forceinline__ void scatter_frame(const ReprojSource &S, uint32_t source, uint32_t chunk, const rpj::Target &tg, uint32_t *__restrict__ keys, uint4 *s_in,
                                              uint32_t (&n)[4])
{
    constexpr uint32_t PER = 16u / sizeof(D);
    union Pack { uint4 q; D e[PER]; };
    const uint32_t t = threadIdx.x;
    const D *data = static_cast<const D *>(S.data);
    const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 15u) / (uint32_t)sizeof(D);      // the elements in front of `data` in its 16 bytes
    const int32_t first = (int32_t)(chunk * kReprojThreads * PER) - (int32_t)off;      // the element of the workgroup's first slot (below 0: in front of the source)
    const int32_t e0 = first + (int32_t)(t * PER);
    Pack in;
    if (e0 >= 0 && e0 + (int32_t)PER <= (int32_t)S.n) in.q = *reinterpret_cast<const uint4 *>(data + e0);      // (on 16 bytes by construction)
    else {
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) { const int32_t e = e0 + (int32_t)k; in.e[k] = (e >= 0 && e < (int32_t)S.n) ? data[e] : (D)0; }
    }
    s_in[t] = in.q;
    __syncthreads();
    const D *s_e = reinterpret_cast<const D *>(s_in);
#pragma unroll 1
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t j = k * kReprojThreads + t;
        const uint32_t d0 = dfilt::depth_of(s_e[j]);
        if (d0 == 0u) continue;                                    // not measured, or no element of the source: no sample
        if (d0 > rpj::kMaxDepth) { n[0] += 1u; n[2] += 1u; continue; }
        const uint32_t e = (uint32_t)(first + (int32_t)j), y = e / S.width, x = e - y * S.width;
        float px, py, pz;
        rpj::frame_point(x, y, d0, S.fx, S.fy, S.cx, S.cy, px, py, pz);
        scatter_sample(S.T, tg, source, px, py, pz, keys, n);
    }
}

// A cloud source: lane t loads points 4 t .. 4 t + 3 of the workgroup's 1024 (three 16-byte loads where the cloud starts on 16 bytes and all four
// exist, float by float otherwise) into LDS; then lane t works on points t, 256 + t, ...
__device__ __forceinline__ void scatter_cloud(const ReprojSource &S, uint32_t source, uint32_t chunk, const rpj::Target &tg, uint32_t *__restrict__ keys, uint4 *s_in,
                                              uint32_t (&n)[4])
{
    const uint32_t t = threadIdx.x;
    const float *data = static_cast<const float *>(S.data);
    const uint32_t first = chunk * kReprojThreads * kRpCloudPer, p0 = first + t * kRpCloudPer;
    union Pack { uint4 q[3]; float f[12]; } in;
    if ((reinterpret_cast<uintptr_t>(data) & 15u) == 0 && p0 + kRpCloudPer <= S.n) {
        const uint4 *src = reinterpret_cast<const uint4 *>(data + (size_t)p0 * 3u);
        in.q[0] = src[0]; in.q[1] = src[1]; in.q[2] = src[2];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) in.f[k] = (p0 + k / 3u < S.n) ? data[(size_t)(p0 + k / 3u) * 3u + k % 3u] : 0.0f;
    }
    s_in[t * 3u] = in.q[0]; s_in[t * 3u + 1u] = in.q[1]; s_in[t * 3u + 2u] = in.q[2];
    __syncthreads();
    const float *s_f = reinterpret_cast<const float *>(s_in);
#pragma unroll 1
    for (uint32_t k = 0; k < kRpCloudPer; ++k) {
        const uint32_t j = k * kReprojThreads + t;
        if (first + j >= S.n) continue;
        scatter_sample(S.T, tg, source, s_f[j * 3u], s_f[j * 3u + 1u], s_f[j * 3u + 2u], keys, n);
    }
}

__global__ __launch_bounds__(kReprojThreads) void reproject_scatter_kernel(ReprojSources src, rpj::Target tg, uint32_t *__restrict__ keys, ReprojControl *ctl)
{
    __shared__ uint4 s_in[kReprojThreads * 3];                     // 12 KiB: the workgroup's 1024 points, or (in its first third) its 256 slots of a frame
    __shared__ uint32_t s_n[4];
    const uint32_t t = threadIdx.x;
    uint32_t si = 0;                                               // the workgroup's source: the last one whose first chunk is not behind it
#pragma unroll
    for (uint32_t i = 1; i < rpj::kMaxSources; ++i) si += (i < src.n_sources && blockIdx.x >= src.s[i].first_block) ? 1u : 0u;
    const ReprojSource &S = src.s[si];
    const uint32_t chunk = blockIdx.x - S.first_block;
    if (t < 4) s_n[t] = 0u;
    uint32_t n[4] = { 0u, 0u, 0u, 0u };
    if (S.kind == PR_SRC_DEPTH_U16) scatter_frame<uint16_t>(S, si, chunk, tg, keys, s_in, n);      // (one source, one kind per workgroup: every lane takes the same branch)
    else if (S.kind == PR_SRC_DEPTH_I32) scatter_frame<int32_t>(S, si, chunk, tg, keys, s_in, n);
    else scatter_cloud(S, si, chunk, tg, keys, s_in, n);
    // the counts: a wavefront's sum, the wavefronts' in LDS, one atomic per counter the workgroup has
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        uint32_t v = n[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((t & 63u) == 0 && v) atomicAdd(&s_n[c], v);
    }
    __syncthreads();
    if (t < 4 && s_n[t]) atomicAdd(&ctl->src[si][t], s_n[t]);
}

// ---- resolve: a workgroup per tile -----------------------------------------------------------------------------------------------------------
// s_z: Z on the tile and two pixels around it (0 outside the frame; not filled when the visibility stage is off, R == 0).  A lane's window is
// (2 R + 1)^2 words at compile-time offsets from its own; rows of 68 words: the lanes of a wavefront read consecutive words.
template <class O, int R>
__global__ __launch_bounds__(kRpTileThreads) void reproject_resolve_kernel(const uint32_t *__restrict__ keys, uint32_t width, uint32_t height, pr_reproject_params prm,
                                                                           O *__restrict__ depth_out, uint8_t *__restrict__ source_out, ReprojControl *ctl,
                                                                           ReprojControl *ctl_out)
{
    __shared__ uint32_t s_z[kRpZW * kRpZH], s_n[11], s_last;       // s_n: won[8], covered, hidden, kept -- ReprojControl's order
    const uint32_t lane = threadIdx.x, row = threadIdx.y, t = row * kRpTileW + lane;
    const int ox = (int)(blockIdx.x * kRpTileW), oy = (int)(blockIdx.y * kRpTileH);
    if (t < 11) s_n[t] = 0u;
    if (R > 0) {
        for (uint32_t c = t; c < kRpZW * kRpZH; c += kRpTileThreads) {
            const int x = ox + (int)(c % kRpZW) - (int)kRpHalo, y = oy + (int)(c / kRpZW) - (int)kRpHalo;
            uint32_t z = 0u;
            if (x >= 0 && y >= 0 && x < (int)width && y < (int)height) z = rpj::depth_of_key(keys[(size_t)y * width + (size_t)x]);
            s_z[c] = z;
        }
    }
    __syncthreads();
    const uint32_t x = (uint32_t)ox + lane, y = (uint32_t)oy + row;
    uint32_t s = 0xFFFFu;                                          // a lane outside the frame counts for nothing
    if (x < width && y < height) {
        const size_t i = (size_t)y * width + x;
        const uint32_t key = keys[i], z0 = rpj::depth_of_key(key);
        const uint32_t zat = (row + kRpHalo) * kRpZW + lane + kRpHalo;
        uint32_t o = 0u;
        s = PR_REPROJECT_NONE;
        if (z0 != 0u) {
            const bool hid = rpj::hidden<R>(prm, z0, [&](int dx, int dy) { return s_z[(int)zat + dy * (int)kRpZW + dx]; });
            o = hid ? 0u : z0;
            s = hid ? (uint32_t)PR_REPROJECT_HIDDEN : (key & 7u);
        }
        depth_out[i] = (O)o;
        if (source_out) source_out[i] = (uint8_t)s;
    }
    // the counts: a wavefront's lanes per counter by ballot, the wavefronts' in LDS, one atomic per counter the tile has
#pragma unroll
    for (uint32_t c = 0; c < 11; ++c) {
        const bool is = c < 8 ? s == c : c == 8 ? (s < 8u || s == PR_REPROJECT_HIDDEN) : c == 9 ? s == PR_REPROJECT_HIDDEN : s < 8u;
        const uint32_t k = (uint32_t)__popcll(__ballot(is));
        if (lane == 0 && k) atomicAdd(&s_n[c], k);
    }
    __syncthreads();
    if (t < 11) {
        if (s_n[t]) atomicAdd(reinterpret_cast<uint32_t *>(ctl) + kRpWonWord + t, s_n[t]);      // (won[8], covered, hidden, kept lie one behind the other)
        __threadfence();                                           // this tile's counts are in place before its ticket is drawn
    }
    __syncthreads();
    if (t == 0) s_last = (atomicAdd(&ctl->done, 1u) == gridDim.x * gridDim.y - 1u) ? 1u : 0u;
    __syncthreads();
    if (s_last != 0u && t < kRpControlWords) {                     // the last tile to arrive: every count of the call is in, and goes to the host's copy
        __threadfence();
        reinterpret_cast<uint32_t *>(ctl_out)[t] = __hip_atomic_load(reinterpret_cast<uint32_t *>(ctl) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
uint32_t reproject_blocks(uint32_t kind, const void *data, uint32_t n)
{
    uint32_t slots;
    if (kind == PR_SRC_CLOUD) slots = (n + kRpCloudPer - 1u) / kRpCloudPer;
    else {
        const uint32_t size = kind == PR_SRC_DEPTH_I32 ? 4u : 2u, per = 16u / size, off = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 15u) / size;
        slots = (off + n + per - 1u) / per;
    }
    return (slots + kReprojThreads - 1u) / kReprojThreads;
}

hipError_t launch_reproject_clear(uint32_t *keys, uint32_t n_px, ReprojControl *ctl, hipStream_t s)
{
    const uint32_t n_threads = n_px / 4u + n_px % 4u;
    hipLaunchKernelGGL(reproject_clear_kernel, dim3((n_threads + kReprojThreads - 1u) / kReprojThreads), dim3(kReprojThreads), 0, s, keys, n_px, ctl);
    return hipGetLastError();
}

hipError_t launch_reproject_scatter(const ReprojSources &src, const rpj::Target &target, uint32_t *keys, ReprojControl *ctl, hipStream_t s)
{
    hipLaunchKernelGGL(reproject_scatter_kernel, dim3(src.n_blocks), dim3(kReprojThreads), 0, s, src, target, keys, ctl);
    return hipGetLastError();
}

hipError_t launch_reproject_resolve(const uint32_t *keys, uint32_t width, uint32_t height, const pr_reproject_params &params, bool out_i32, void *depth_out,
                                    uint8_t *source_out, ReprojControl *ctl, ReprojControl *ctl_out, hipStream_t s)
{
    const dim3 grid((width + kRpTileW - 1) / kRpTileW, (height + kRpTileH - 1) / kRpTileH), block(kRpTileW, kRpTileH);
    const uint32_t r = params.occl_min_front == 0u ? 0u : params.occl_radius;      // (the stage off: no window, whatever the radius)
    for_depth_type(out_i32, [&](auto *tag) {
        using O = std::remove_pointer_t<decltype(tag)>;
        O *out = static_cast<O *>(depth_out);
        if (r == 0) hipLaunchKernelGGL((reproject_resolve_kernel<O, 0>), grid, block, 0, s, keys, width, height, params, out, source_out, ctl, ctl_out);
        else if (r == 1) hipLaunchKernelGGL((reproject_resolve_kernel<O, 1>), grid, block, 0, s, keys, width, height, params, out, source_out, ctl, ctl_out);
        else hipLaunchKernelGGL((reproject_resolve_kernel<O, 2>), grid, block, 0, s, keys, width, height, params, out, source_out, ctl, ctl_out);
    });
    return hipGetLastError();
}

}  // namespace prk
