// raster.hip -- render_triangle + rasterization (cuda_renderer/renderer.cu:83-187) for a batch of hypotheses: clear, per-hypothesis pixel boxes, triangle raster with int32 atomicMin, row counts
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"
#define PR_HD __host__ __device__
#include "pose_box.h"

namespace prk {

// ================================================================================================
//  fill / max2zero
// ================================================================================================
__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t *dst, size_t n, int32_t v)
{
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (; i + 3 < n; i += stride) *reinterpret_cast<int4 *>(dst + i) = make_int4(v, v, v, v);
    if (i < n) for (size_t k = i; k < n && k < i + 4; ++k) dst[k] = v;
}

// renderer.cu:71-80 max2zero_functor over the whole stack of images: "nothing drawn" (kSentinel: INT_MAX in a near plane, INT_MIN in the far plane
// of a span render) to 0.  Both carry the name bench.py's counter calibration and tools/gpu_round.sh select by.
template <int32_t kSentinel>
__global__ __launch_bounds__(256) void max2zero_kernel(int32_t *d, size_t n)
{
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (; i + 3 < n; i += stride) {
        int4 v = *reinterpret_cast<int4 *>(d + i);
        v.x = (v.x == kSentinel) ? 0 : v.x; v.y = (v.y == kSentinel) ? 0 : v.y;
        v.z = (v.z == kSentinel) ? 0 : v.z; v.w = (v.w == kSentinel) ? 0 : v.w;
        *reinterpret_cast<int4 *>(d + i) = v;
    }
    if (i < n) for (size_t k = i; k < n && k < i + 4; ++k) if (d[k] == kSentinel) d[k] = 0;
}

// ================================================================================================
//  triangle raster: one lane = one (triangle, hypothesis); int32 atomicMin resolves depth
// ================================================================================================
__device__ __forceinline__ float area2(float ax, float ay, float bx, float by, float cx, float cy)
{   // renderer.h:315-318 calculateSignedArea
    return 0.5f * ((cx - ax) * (by - ay) - (bx - ax) * (cy - ay));
}

// Per-triangle screen-space setup shared by the raster kernels: model + projection + viewport
// transform (renderer.cu:159-186, :90-98), clamped pixel box (:100-122), signed area (renderer.h:315-333).
struct TriSetup {
    float px[3], py[3], w3[3];
    float base_inv;
    int x0, y0, nx, ny;          // first pixel column/row of the loops of renderer.cu:124-125 and their trip counts
};
__device__ __forceinline__ int trip_count(int first, float hi)
{   // number of iterations of  for (p = first; (float)p <= hi; ++p)  with first in [0, 2^24) or INT_MAX
    if (first == INT_MAX || !(hi >= (float)first)) return 0;
    return (int)floorf(hi) - first + 1;
}
__device__ __forceinline__ void tri_setup(const float *__restrict__ tv, const float *__restrict__ M, const pr_mat4 &proj,
                                          uint32_t width, uint32_t height, float cmin0, float cmin1, float cmax0, float cmax1,
                                          TriSetup &t)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // model, projection and viewport transform (vertex_to_screen, pose_box.h: shared with the tight pixel box)
        const ScreenVertex s = vertex_to_screen(tv[3 * k], tv[3 * k + 1], tv[3 * k + 2], M, proj, width, height);
        t.w3[k] = s.lz;                                          // renderer.cu:177-183 last_row
        t.px[k] = s.px;
        t.py[k] = s.py;
    }
    float lo0 = FLT_MAX, lo1 = FLT_MAX, hi0 = -FLT_MAX, hi1 = -FLT_MAX;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo0 = sel_max(cmin0, sel_min(lo0, t.px[k]));  hi0 = sel_min(cmax0, sel_max(hi0, t.px[k]));
        lo1 = sel_max(cmin1, sel_min(lo1, t.py[k]));  hi1 = sel_min(cmax1, sel_max(hi1, t.py[k]));
    }
    const float area = area2(t.px[0], t.py[0], t.px[1], t.py[1], t.px[2], t.py[2]);
    t.x0 = loop_start(lo0 + 0.5f);
    t.y0 = loop_start(lo1 + 0.5f);
    t.nx = trip_count(t.x0, hi0);
    t.ny = trip_count(t.y0, hi1);
    if (!(area != 0.0f)) { t.nx = 0; t.ny = 0; }                 // documented: zero-area triangles are skipped
    t.base_inv = 1 / area;
}
// one candidate pixel of one triangle: barycentric test + perspective depth (renderer.cu:126-140)
__device__ __forceinline__ bool tri_fragment(const float px[3], const float py[3], float base_inv, int x, int y,
                                             float &alpha, float &beta, float &gamma)
{
    const float fx = (float)x, fy = (float)y;
    beta  = area2(px[0], py[0], fx, fy, px[2], py[2]) * base_inv;
    gamma = area2(px[0], py[0], px[1], py[1], fx, fy) * base_inv;
    alpha = 1.0f - beta - gamma;
    return !(alpha < -0.0f || beta < -0.0f || gamma < -0.0f || alpha > 1.0f || beta > 1.0f || gamma > 1.0f);
}
// the same test with the triangle's two edge vectors from vertex 0 formed once per triangle (e1 = p1 - p0, e2 = p2 - p0: the very subtractions area2 makes per
// pixel, so every product and difference below is the same float as in tri_fragment)
__device__ __forceinline__ bool tri_fragment_edges(float px0, float py0, float e1x, float e1y, float e2x, float e2y, float base_inv, int x, int y,
                                                   float &alpha, float &beta, float &gamma)
{
    const float dx = (float)x - px0, dy = (float)y - py0;
    beta  = 0.5f * (e2x * dy - dx * e2y) * base_inv;               // area2(p0, f, p2) * base_inv
    gamma = 0.5f * (dx * e1y - e1x * dy) * base_inv;               // area2(p0, p1, f) * base_inv
    alpha = 1.0f - beta - gamma;
    return !(alpha < -0.0f || beta < -0.0f || gamma < -0.0f || alpha > 1.0f || beta > 1.0f || gamma > 1.0f);
}
__device__ __forceinline__ int fragment_depth(float alpha, float beta, float gamma, float w0, float w1, float w2)
{
    const float az = alpha / w0, bz = beta / w1, gz = gamma / w2;
    const float frag = (alpha + beta + gamma) / (az + bz + gz);
    return f2i_x86(frag + 0.5f);
}

// Wave-cooperative raster of up to 64 set-up triangles (one per lane, n = candidate pixels of the lane's triangle, 0 for none).
// Thread-per-triangle pixel loops waste most lanes (the average triangle of obj_06 tests 7 pixel centres, the largest 36), so
// the wavefront expands its triangles into one dense list of candidate pixels (exclusive scan of the per-triangle counts) and
// walks that list 64 candidates at a time: every lane finds the owner of its candidate by a 6-step search over the scanned
// offsets and reads the owner's setup back from LDS.  Candidates that pass the inside test are rare (about one in four) --
// they are queued per wavefront as packed (owner, x, y) words and drained 64 at a time, so the four IEEE divisions of the
// perspective depth and the depth update (`sink(x, y, depth)`) always run on full wavefronts.  Same arithmetic per candidate
// as renderer.cu:124-140.  `w` / `queue` are this wavefront's private LDS scratch.
constexpr int kSetupWords = 15;
template <class Sink>
__device__ __forceinline__ void wave_raster(const TriSetup &t, int n, float (*w)[64], uint32_t *queue, Sink sink)
{
    const uint32_t lane = threadIdx.x & 63;
    // exclusive scan of n over the wavefront
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off); if ((int)lane >= off) incl += v; }
    const int excl = incl - n;
    const int total = __shfl(incl, 63);

    w[0][lane] = t.px[0]; w[1][lane] = t.py[0]; w[2][lane] = t.px[1] - t.px[0]; w[3][lane] = t.py[1] - t.py[0]; w[4][lane] = t.px[2] - t.px[0]; w[5][lane] = t.py[2] - t.py[0];
    w[6][lane] = t.w3[0]; w[7][lane] = t.w3[1]; w[8][lane] = t.w3[2]; w[9][lane] = t.base_inv;
    w[10][lane] = __int_as_float(t.x0); w[11][lane] = __int_as_float(t.y0); w[12][lane] = __int_as_float(t.nx > 0 ? t.nx : 1);
    w[13][lane] = __int_as_float(excl);
    w[14][lane] = __builtin_amdgcn_rcpf((float)(t.nx > 0 ? t.nx : 1));
    // wavefronts only touch their own slice; a wave-level fence is enough for LDS ordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // The owner of candidate c = the last triangle whose run starts at or before c.  Round 6: instead of a six-step search over the scanned offsets (six
    // dependent LDS reads per candidate), the triangles whose runs start inside the current window of 64 candidates mark their first slot with lane + 1
    // and an inclusive maximum over the lanes (four row shifts + two row broadcasts, no LDS) carries each mark to the end of its run; a run that began in
    // an earlier window arrives through `carry`, the owner of that window's last candidate.
    uint32_t *mark = queue + 128;
    int carry = 0;
    int qn = 0;                                                    // wave-uniform fill level, < 64 between iterations
    auto drain = [&](int first, int count) {
        if ((int)lane < count) {
            const uint32_t e = queue[first + lane];
            const int o = (int)(e >> 26), x = (int)((e >> 13) & 0x1fffu), y = (int)(e & 0x1fffu);
            float alpha, beta, gamma;
            (void)tri_fragment_edges(w[0][o], w[1][o], w[2][o], w[3][o], w[4][o], w[5][o], w[9][o], x, y, alpha, beta, gamma);
            sink(x, y, fragment_depth(alpha, beta, gamma, w[6][o], w[7][o], w[8][o]));
        }
    };
    for (int c0 = 0; c0 < total; c0 += 64) {
        const int c = c0 + (int)lane;
        bool pass = false;
        uint32_t entry = 0;
        mark[lane] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (n > 0 && excl >= c0 && excl < c0 + 64) mark[excl - c0] = lane + 1u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int own = (int)mark[lane];
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x111, 0xf, 0xf, true));      // row_shr:1
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x112, 0xf, 0xf, true));      // row_shr:2
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x114, 0xf, 0xf, true));      // row_shr:4
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x118, 0xf, 0xf, true));      // row_shr:8
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x142, 0xa, 0xf, true));      // row_bcast15 -> rows 1, 3
        own = max(own, __builtin_amdgcn_update_dpp(0, own, 0x143, 0xc, 0xf, true));      // row_bcast31 -> rows 2, 3
        own = max(own, carry);
        carry = __builtin_amdgcn_readlane(own, 63);                 // (only used when another window follows: lane 63 then held a real candidate)
        if (c < total) {
            const int o = own - 1;
            const int k = c - __float_as_int(w[13][o]);
            const int nx = __float_as_int(w[12][o]);
            // k / nx from the owner's reciprocal with a one-step correction; k, nx, q*nx < 2^24 (a frame has < 2^24 pixels),
            // so the 24-bit multiplier (full rate, v_mul_lo_u32 is quarter rate) is exact
            int q = (int)((float)k * w[14][o]);
            if ((int)__umul24((unsigned)q, (unsigned)nx) > k) --q;
            if ((int)__umul24((unsigned)(q + 1), (unsigned)nx) <= k) ++q;
            const int x = __float_as_int(w[10][o]) + (k - (int)__umul24((unsigned)q, (unsigned)nx));
            const int y = __float_as_int(w[11][o]) + q;
            float alpha, beta, gamma;
            pass = tri_fragment_edges(w[0][o], w[1][o], w[2][o], w[3][o], w[4][o], w[5][o], w[9][o], x, y, alpha, beta, gamma);
            entry = ((uint32_t)o << 26) | ((uint32_t)x << 13) | (uint32_t)y;
        }
        const unsigned long long m = __ballot(pass);
        if (pass) queue[qn + (int)__popcll(m & ((1ull << lane) - 1ull))] = entry;
        qn += (int)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64) { drain(qn - 64, 64); qn -= 64; __builtin_amdgcn_wave_barrier(); }
    }
    drain(0, qn);
    __builtin_amdgcn_wave_barrier();                             // the scratch may be refilled by the caller's next chunk
}

// one lane = one (triangle, hypothesis); depth resolved with int32 atomicMin in global memory (the reference scheme).
__device__ __forceinline__ uint32_t f32_key(float v) { const uint32_t b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// A mesh box kept as six keys {minx,miny,minz,maxx,maxy,maxz}: a float maps to a key that orders like the float (sign bit flipped for
// positives, all bits for negatives); minima store the key, maxima its complement, so all six start from 0xffffffff and merge with
// atomicMin.  box_key_merge: the workgroup's lane minima / maxima into keys[0..5] (red: 4 x 6 floats of LDS).
__device__ __forceinline__ void box_key_merge(float (&lo)[3], float (&hi)[3], float (*red)[6], uint32_t *keys)
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int off = 32; off > 0; off >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], off)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off)); }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) for (int a = 0; a < 3; ++a) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) { const float o = red[w][threadIdx.x]; r = (threadIdx.x < 3) ? fminf(r, o) : fmaxf(r, o); }
        atomicMin(&keys[threadIdx.x], (threadIdx.x < 3) ? f32_key(r) : ~f32_key(r));
    }
}
// key k of box word a back to its float; a key no vertex reached (an empty mesh) stays +FLT_MAX / -FLT_MAX
__device__ __forceinline__ float box_key_value(uint32_t k, uint32_t a)
{
    float v = key_f32((a < 3) ? k : ~k);
    if (k == 0xffffffffu) v = (a < 3) ? FLT_MAX : -FLT_MAX;
    return v;
}
// The per-batch safety nets, carried by the raster (BatchCheck, pr_internal.h): called by the workgroups of the launch's first hypothesis with
// the CALLER's triangles of their 256 places in registers (the raster itself may read the library's ordered copy).  `red` / `part`: LDS
// scratch (6 x 4 floats, 16 words: [0..3] scene fingerprint, [4] ticket, [8..15] the wavefronts' mesh fingerprint sums as lo / hi words).
__device__ __forceinline__ void raster_batch_check(const float (&tv)[9], bool have, const BatchCheck &chk, float (*red)[6], uint32_t *part)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {   // multiset fingerprint of the caller's buffer: this workgroup's share (read by thread 0 after box_key_merge's barrier)
        uint32_t w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = __float_as_uint(tv[k]);
        unsigned long long h = have ? triangle_hash(w) : 0ull;
        for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
        if (lane == 0) { part[8 + 2 * wave] = (uint32_t)h; part[9 + 2 * wave] = (uint32_t)(h >> 32); }
    }
    if (blockIdx.x == 0 && chk.fp_expected) {
        uint32_t h = fingerprint_lane(chk.fa, chk.na, chk.fb, chk.nb, chk.fc, chk.nc);
        for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
        if (lane == 0) part[wave] = h;
        __syncthreads();
        if (threadIdx.x == 0 && *chk.fp_expected != part[0] + part[1] + part[2] + part[3]) *chk.flag = 1u;
        __syncthreads();
    }
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = have ? fminf(fminf(tv[a], tv[3 + a]), tv[6 + a]) : FLT_MAX;
        hi[a] = have ? fmaxf(fmaxf(tv[a], tv[3 + a]), tv[6 + a]) : -FLT_MAX;
    }
    box_key_merge(lo, hi, red, chk.keys);
    unsigned long long *mesh_sum = reinterpret_cast<unsigned long long *>(chk.keys + 8);
    if (threadIdx.x == 0) {
        unsigned long long h = 0;
        for (int w = 0; w < 4; ++w) h += (unsigned long long)part[8 + 2 * w] | ((unsigned long long)part[9 + 2 * w] << 32);
        atomicAdd(mesh_sum, h);
    }
    if (threadIdx.x < 6) __threadfence();                            // this workgroup's minima and its share of the sum are in place before its ticket is drawn
    __syncthreads();
    if (threadIdx.x == 0) part[4] = (atomicAdd(&chk.keys[6], 1u) == gridDim.x - 1u) ? 1u : 0u;
    __syncthreads();
    if (part[4] != 0u && threadIdx.x == 0) {                         // the last workgroup to arrive: compare, and re-arm the words for the next batch
        __threadfence();
        bool differs = false;
        for (uint32_t a = 0; a < 6; ++a)
            if (!(box_key_value(atomicExch(&chk.keys[a], 0xffffffffu), a) == chk.expect.v[a])) differs = true;
        if (atomicExch(mesh_sum, 0ull) != chk.mesh_hash) differs = true;
        atomicExch(&chk.keys[6], 0u);
        if (differs) *chk.flag = 1u;
    }
    __syncthreads();
}

// the lane's triangle of a raster workgroup (zeros past the end of the mesh)
__device__ __forceinline__ void load_triangle(const pr_triangle *__restrict__ tris, uint32_t n_tris, uint32_t ti, float (&tv)[9])
{
    if (ti < n_tris) {
        const float *src = reinterpret_cast<const float *>(tris + ti);
#pragma unroll
        for (int k = 0; k < 9; ++k) tv[k] = src[k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) tv[k] = 0.0f;
    }
}

// What one raster workgroup does with its 256 triangles (tv, lane triangle ti of n_tris): hypotheses [run * pose_run, +pose_run) of the
// n_poses at `poses`.  Image of hypothesis `by`: depth + image_of[by] * rw * rh when image_of is given (the caller's order of a mixed
// batch), depth + by * rw * rh otherwise; packed boxes (box_off): their own pitch, or -- kBands, the asynchronous fused path's option box_bands --
// the banded layout of pose_box.h (band_box), whose per-hypothesis constants are folded into the base as the row-major origin is.
// kSpan (the span kernels below; never with kBands): `far` is a second plane of the same layout, and every fragment's depth also goes
// into it with atomicMax -- the farthest fragment of the pixel from the very int32 the nearest is taken from.
template <bool kBands, bool kSpan = false>
__device__ __forceinline__ void raster_runs(const float (&tv)[9], uint32_t ti, uint32_t n_tris, uint32_t run,
                                            const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth,
                                            uint32_t width, uint32_t height, const pr_mat4 &proj, pr_roi roi,
                                            uint32_t rw, uint32_t rh, const int4 *__restrict__ boxes, uint32_t n_poses, uint32_t pose_run,
                                            const uint32_t *__restrict__ box_off, const uint32_t *__restrict__ image_of,
                                            float (*sh)[kSetupWords][64], uint32_t (*shq)[192], int32_t *__restrict__ far = nullptr)
{
    static_assert(!(kBands && kSpan), "the span render uses row-major boxes");
    const uint32_t wave = threadIdx.x >> 6;
    float rmin0 = 0.0f, rmin1 = 0.0f, rmax0 = (float)(width - 1), rmax1 = (float)(height - 1);
    if (roi.width > 0 && roi.height > 0) {                       // renderer.cu:106-113 (image is flipped in y)
        rmin0 = (float)roi.x;
        rmin1 = (float)((unsigned long long)(height - 1) - (unsigned long long)(long long)(roi.y + roi.height - 1));
        rmax0 = (float)((roi.x + roi.width) - 1);
        rmax1 = (float)((unsigned long long)(height - 1) - (unsigned long long)(long long)roi.y);
    }
    for (uint32_t k = 0; k < pose_run; ++k) {
        const uint32_t by = run * pose_run + k;
        if (by >= n_poses) break;
        const float *M = poses[by].m;                            // wave-uniform -> scalar loads
        int32_t *img = depth + (size_t)(image_of ? image_of[by] : by) * rw * rh;
        float cmin0 = rmin0, cmin1 = rmin1, cmax0 = rmax0, cmax1 = rmax1;
        uint32_t pitch = rw;                                     // image row pitch; packed boxes (box_off): the box's own width, origin at its top-left pixel
        if (boxes) {                                             // fused path: the hypothesis' pixel box (already intersected with the caller's ROI,
            const int4 bb = boxes[by];                           // if any); a conservative box clips nothing, an ROI clips like renderer.cu:106-113
            cmin0 = (float)bb.x; cmin1 = (float)bb.y; cmax0 = (float)bb.z; cmax1 = (float)bb.w;
            if constexpr (kBands) {
                const BandBox k = band_box(bb, height);
                pitch = (uint32_t)k.w;
                img = depth + box_off[by] + band_origin(k, bb);
            } else if (box_off) {
                pitch = (uint32_t)max(bb.z - bb.x + 1, 0);
                // pixel (x, image row r) of the box lives at off + (r - r0) * pitch + (x - bb.x), r0 = height - 1 - bb.w: fold the origin into the base
                img = depth + box_off[by] - ((ptrdiff_t)((int)height - 1 - bb.w) * (ptrdiff_t)pitch + (ptrdiff_t)bb.x);
            }
        }
        TriSetup t;
        int n = 0;
        if (ti < n_tris) {
            tri_setup(tv, M, proj, width, height, cmin0, cmin1, cmax0, cmax1, t);
            n = t.nx * t.ny;
        } else { t.nx = t.ny = 0; t.x0 = t.y0 = 0; t.base_inv = 0; for (int j = 0; j < 3; ++j) t.px[j] = t.py[j] = t.w3[j] = 0; }
        wave_raster(t, n, sh[wave], shq[wave], [&](int x, int y, int d) {
            if constexpr (kBands) {                              // (launched with packed boxes and no ROI of its own: the fragment lies inside bb)
                atomicMin(&img[band_index(pitch, (uint32_t)x, height - 1u - (uint32_t)y)], d);
            } else {
                const uint32_t xw = (uint32_t)(x - roi.x);
                const uint32_t yw = (uint32_t)((int)height - 1 - y - roi.y);
                atomicMin(&img[xw + (size_t)yw * pitch], d);
                if constexpr (kSpan) atomicMax(&far[(img - depth) + (ptrdiff_t)(xw + (size_t)yw * pitch)], d);
            }
        });
    }
}

// A workgroup keeps its 256 triangles in registers and walks `pose_run` consecutive hypotheses with them: a mesh that does not fit
// the L2 (the 1 M-triangle mesh of BASELINE configs[4]: 36 MB) is then streamed from the Infinity Cache / HBM once per pose_run
// hypotheses instead of once per hypothesis -- at 128 hypotheses that stream (4.6 GB, 3.2 TB/s) was what bounded the kernel.
template <bool kBands>
__global__ __launch_bounds__(256) void raster_kernel(const pr_triangle *__restrict__ tris, uint32_t n_tris,
                                                     const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth,
                                                     uint32_t width, uint32_t height, pr_mat4 proj, pr_roi roi,
                                                     uint32_t rw, uint32_t rh, const int4 *__restrict__ boxes, uint32_t n_poses, uint32_t pose_run,
                                                     const uint32_t *__restrict__ box_off, BatchCheck chk)
{
    __shared__ float sh[4][kSetupWords][64];
    __shared__ uint32_t shq[4][192];                              // per wavefront: 128 words of fragment queue, 64 of run marks (wave_raster)
    const uint32_t ti = blockIdx.x * 256 + threadIdx.x;
    float tv[9];
    load_triangle(tris, n_tris, ti, tv);
    if (chk.keys && blockIdx.y == 0) {                           // (wave-uniform) the asynchronous path's per-batch checks ride on the first hypothesis' workgroups
        float cv[9];                                             // ... and look at the caller's buffer: `tris` may be the library's ordered copy of it
        load_triangle(chk.caller, n_tris, ti, cv);
        raster_batch_check(cv, ti < n_tris, chk, reinterpret_cast<float (*)[6]>(&sh[0][0][0]), &shq[0][0]);
    }
    raster_runs<kBands>(tv, ti, n_tris, blockIdx.y, poses, depth, width, height, proj, roi, rw, rh, boxes, n_poses, pose_run, box_off, nullptr, sh, shq);
}

// A mixed batch (hypotheses of several meshes) in one launch.  The hypotheses come grouped by mesh; group g owns the 1-D workgroup
// range [first_wg, first_wg + tri_blocks * ceil(count / run)) and each of its workgroups does exactly what raster_kernel's workgroup
// (triangle block, pose run) does for that group's mesh and hypotheses -- so a 1 M-triangle mesh next to 5 k-triangle ones launches
// no empty workgroups, and every depth is the same atomicMin of the same fragment as in a single-mesh launch.  The group of a workgroup:
// a wave-uniform binary search over the groups' first workgroups (scalar loads).  Workgroups beyond the grid loop (64-bit totals).
// kSpan: raster_runs' second plane, `far`, laid out as `depth`.
template <bool kSpan>
__device__ __forceinline__ void raster_group_walk(const RasterGroup *__restrict__ groups, uint32_t n_groups, unsigned long long total_wg,
                                                  const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth, int32_t *__restrict__ far,
                                                  uint32_t width, uint32_t height, const pr_mat4 &proj, pr_roi roi, uint32_t rw, uint32_t rh,
                                                  const int4 *__restrict__ boxes, const uint32_t *__restrict__ box_off,
                                                  const uint32_t *__restrict__ image_of, float (*sh)[kSetupWords][64], uint32_t (*shq)[192])
{
    for (unsigned long long wg = blockIdx.x; wg < total_wg; wg += gridDim.x) {
        uint32_t lo = 0, hi = n_groups;                          // groups[lo].first_wg <= wg < groups[hi].first_wg
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (groups[mid].first_wg <= wg) lo = mid; else hi = mid;
        }
        lo = __builtin_amdgcn_readfirstlane(lo);
        const RasterGroup &gr = groups[lo];
        const unsigned long long local = wg - gr.first_wg;
        const uint32_t run = (uint32_t)(local / gr.tri_blocks), block = (uint32_t)(local - (unsigned long long)run * gr.tri_blocks);
        const uint32_t ti = block * 256 + threadIdx.x;
        float tv[9];
        load_triangle(gr.tris, gr.n_tris, ti, tv);
        // full frames without a caller order: the group's images follow one another from its first hypothesis on
        const size_t first = (image_of || box_off) ? 0 : (size_t)gr.first * rw * rh;
        raster_runs<false, kSpan>(tv, ti, gr.n_tris, run, poses + gr.first, depth + first, width, height, proj, roi, rw, rh, boxes ? boxes + gr.first : nullptr,
                                  gr.count, gr.run, box_off ? box_off + gr.first : nullptr, image_of ? image_of + gr.first : nullptr, sh, shq,
                                  kSpan ? far + first : nullptr);
    }
}
__global__ __launch_bounds__(256) void raster_multi_kernel(const RasterGroup *__restrict__ groups, uint32_t n_groups, unsigned long long total_wg,
                                                           const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth,
                                                           uint32_t width, uint32_t height, pr_mat4 proj, pr_roi roi, uint32_t rw, uint32_t rh,
                                                           const int4 *__restrict__ boxes, const uint32_t *__restrict__ box_off,
                                                           const uint32_t *__restrict__ image_of)
{
    __shared__ float sh[4][kSetupWords][64];
    __shared__ uint32_t shq[4][192];
    raster_group_walk<false>(groups, n_groups, total_wg, poses, depth, nullptr, width, height, proj, roi, rw, rh, boxes, box_off, image_of, sh, shq);
}

// The span forms of raster_kernel<false> and raster_multi_kernel (pr_render_span, pr_pose_penetration): the same workgroups, triangles, hypotheses
// and fragments, every depth into two planes of one layout -- atomicMin into `depth`, atomicMax into `far` (full frames or packed boxes; a mixed
// batch's full frames are never span renders, so its form has no image_of).
__global__ __launch_bounds__(256) void raster_span_kernel(const pr_triangle *__restrict__ tris, uint32_t n_tris,
                                                          const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth, int32_t *__restrict__ far,
                                                          uint32_t width, uint32_t height, pr_mat4 proj, pr_roi roi,
                                                          uint32_t rw, uint32_t rh, const int4 *__restrict__ boxes, uint32_t n_poses, uint32_t pose_run,
                                                          const uint32_t *__restrict__ box_off)
{
    __shared__ float sh[4][kSetupWords][64];
    __shared__ uint32_t shq[4][192];
    const uint32_t ti = blockIdx.x * 256 + threadIdx.x;
    float tv[9];
    load_triangle(tris, n_tris, ti, tv);
    raster_runs<false, true>(tv, ti, n_tris, blockIdx.y, poses, depth, width, height, proj, roi, rw, rh, boxes, n_poses, pose_run, box_off, nullptr, sh, shq, far);
}
__global__ __launch_bounds__(256) void raster_span_multi_kernel(const RasterGroup *__restrict__ groups, uint32_t n_groups, unsigned long long total_wg,
                                                                const pr_mat4 *__restrict__ poses, int32_t *__restrict__ depth, int32_t *__restrict__ far,
                                                                uint32_t width, uint32_t height, pr_mat4 proj, pr_roi roi, uint32_t rw, uint32_t rh,
                                                                const int4 *__restrict__ boxes, const uint32_t *__restrict__ box_off)
{
    __shared__ float sh[4][kSetupWords][64];
    __shared__ uint32_t shq[4][192];
    raster_group_walk<true>(groups, n_groups, total_wg, poses, depth, far, width, height, proj, roi, rw, rh, boxes, box_off, nullptr, sh, shq);
}

// ================================================================================================
//  fused-path raster: per-hypothesis screen bounding box + LDS depth bands (no global atomics, no
//  full-frame clear).  The depth values are produced by exactly the arithmetic of raster_kernel;
//  only where the min is taken (LDS ds_min instead of L2/memory atomics) and which pixels are
//  touched (the conservative box of the object instead of the whole frame) differ.
// ================================================================================================

// axis-aligned box of the mesh in six keys (box_key_merge).  Any number of workgroups: each reduces a slice and merges it; the keys
// start from 0xffffffff (one memset).
__global__ __launch_bounds__(256) void model_aabb_kernel(const pr_triangle *__restrict__ tris, uint32_t n_tris, uint32_t *__restrict__ keys)
{
    __shared__ float red[4][6];
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    const float *v = reinterpret_cast<const float *>(tris);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_tris * 3u; i += gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float c = v[(size_t)i * 3 + a]; lo[a] = fminf(lo[a], c); hi[a] = fmaxf(hi[a], c); }
    }
    box_key_merge(lo, hi, red, keys);
}
// keys -> floats (aabb_out, optional) and/or a check against the box the host assumed (flag_out, optional: 1 = differs)
__global__ void model_aabb_finish_kernel(const uint32_t *__restrict__ keys, float *__restrict__ aabb_out, AabbExpected expect, uint32_t *__restrict__ flag_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool differs = false;
    for (uint32_t a = 0; a < 6; ++a) {
        const float v = box_key_value(keys[a], a);
        if (aabb_out) aabb_out[a] = v;
        if (!(v == expect.v[a])) differs = true;
    }
    if (flag_out) *flag_out = differs ? 1u : 0u;
}
// The boxes of several meshes in one launch: blockIdx.y (grid-stride) = mesh, keys[6 * mesh ...] in model_aabb_kernel's encoding.
// Minima and maxima are exact in any order, so each box equals model_aabb_kernel's for that mesh alone.
__global__ __launch_bounds__(256) void model_aabb_multi_kernel(const pr_mesh_ref *__restrict__ meshes, uint32_t n_meshes, uint32_t *__restrict__ keys)
{
    __shared__ float red[4][6];
    for (uint32_t m = blockIdx.y; m < n_meshes; m += gridDim.y) {
        const float *v = reinterpret_cast<const float *>(meshes[m].tris_dev);
        const uint32_t n_tris = (uint32_t)meshes[m].n_tris;
        float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_tris * 3u; i += gridDim.x * 256) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { const float c = v[(size_t)i * 3 + a]; lo[a] = fminf(lo[a], c); hi[a] = fmaxf(hi[a], c); }
        }
        box_key_merge(lo, hi, red, keys + 6 * (size_t)m);
        __syncthreads();                                             // red is rewritten for the next mesh
    }
}
// keys -> floats, one lane per (mesh, axis)
__global__ __launch_bounds__(256) void model_aabb_multi_finish_kernel(const uint32_t *__restrict__ keys, uint32_t n_words, float *__restrict__ aabb_out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    aabb_out[i] = box_key_value(keys[i], i % 6);
}

// the pixel box of every pose (pose_pixel_box, pose_box.h)
__global__ __launch_bounds__(256) void pose_bbox_kernel(const float *__restrict__ aabb, const pr_mat4 *__restrict__ poses, uint32_t n_poses,
                                                        pr_mat4 proj, uint32_t width, uint32_t height, pr_roi roi, int4 *__restrict__ bbox)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_poses) return;
    bbox[p] = pose_pixel_box(aabb, poses[p].m, proj, width, height, roi);
}
// the same box for a mixed batch: hypothesis p uses the box of its own mesh, aabbs[6 * box_index[p] ...]
__global__ __launch_bounds__(256) void pose_bbox_multi_kernel(const float *__restrict__ aabbs, const uint32_t *__restrict__ box_index,
                                                              const pr_mat4 *__restrict__ poses, uint32_t n_poses, pr_mat4 proj, uint32_t width,
                                                              uint32_t height, pr_roi roi, int4 *__restrict__ bbox)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_poses) return;
    bbox[p] = pose_pixel_box(aabbs + 6 * (size_t)box_index[p], poses[p].m, proj, width, height, roi);
}

// The tight pixel box of every hypothesis (tight_pixel_box, pose_box.h; asynchronous path, option tight_box): one workgroup per hypothesis
// walks the mesh's distinct vertices (`verts`: {x, y, z, 0} each, ensure_model_box) through vertex_to_screen -- the floats the raster's
// triangle setup forms for the same vertex -- and overwrites bbox[hypothesis], which holds the LOOSE box the host sized the batch with, by
// its intersection with the hull of the projected vertices.  Only ever smaller than the loose box: every offset, pitch and capacity derived
// from the loose boxes stays an upper bound.  Lane minima / maxima merged like box_key_merge (wave shuffles, then LDS over the waves).
// 1024 lanes (four waves per SIMD) with four loads in flight each: a lane's chain is a 16-byte load out of L2, then two IEEE divisions that
// depend on it.  By instruction count the launch is ~6 us of issue time for 256 hypotheses of obj_06's 15 736 vertices; traced it takes 12 us
// when it has the chip and 32 us on average beside the other slot's passes (profiles/tight_box; as 256 lanes with one load in flight: 35.5 us).
// A lane past the end re-reads the last vertex: minima, maxima and the flag do not change.
constexpr uint32_t kTightLanes = 1024, kTightLoads = 4;
__global__ __launch_bounds__(kTightLanes) void pose_tight_box_kernel(const float4 *__restrict__ verts, uint32_t n_verts, const pr_mat4 *__restrict__ poses,
                                                                     pr_mat4 proj, uint32_t width, uint32_t height, int4 *__restrict__ bbox)
{
    __shared__ TightAcc red[kTightLanes / 64];
    const float *M = poses[blockIdx.x].m;                            // wave-uniform -> scalar loads
    TightAcc a = tight_acc_empty();
    for (uint32_t i0 = threadIdx.x; i0 < n_verts; i0 += kTightLanes * kTightLoads) {
        float4 v[kTightLoads];
#pragma unroll
        for (uint32_t k = 0; k < kTightLoads; ++k) v[k] = verts[min(i0 + k * kTightLanes, n_verts - 1u)];
#pragma unroll
        for (uint32_t k = 0; k < kTightLoads; ++k) tight_acc_add(a, vertex_to_screen(v[k].x, v[k].y, v[k].z, M, proj, width, height));
    }
    for (int off = 32; off > 0; off >>= 1) {
        TightAcc o;
        o.mnx = __shfl_xor(a.mnx, off); o.mny = __shfl_xor(a.mny, off); o.mxx = __shfl_xor(a.mxx, off); o.mxy = __shfl_xor(a.mxy, off);
        o.bad = __shfl_xor(a.bad, off);
        tight_acc_merge(a, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kTightLanes / 64; ++w) tight_acc_merge(a, red[w]);
        bbox[blockIdx.x] = tight_pixel_box(a, bbox[blockIdx.x]);
    }
}

// INT_MAX-fill and per-row valid counts restricted to each hypothesis' pixel box (image rows are
// the flipped raster rows).  One wavefront per image row; rows outside the box only write count 0.
// kFar: the two planes of a span render -- INT_MAX into the near box, INT_MIN into the far one.
template <bool kFar>
__device__ __forceinline__ void fill_box_rows(int32_t *__restrict__ depth, int32_t *__restrict__ far, const int4 *__restrict__ bbox, uint32_t width,
                                              uint32_t height, const uint32_t *__restrict__ box_off)
{
    const uint32_t lane = threadIdx.x & 63;
    const int4 bb = bbox[blockIdx.y];
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = blockIdx.x * kBoxRowsPerBlock + (threadIdx.x >> 6) * 4 + r;
        if (row >= height) return;
        const int ry = (int)height - 1 - (int)row;                  // raster row of this image row
        if (ry < bb.y || ry > bb.w) continue;
        int32_t *line = box_line(depth, box_off, bb, blockIdx.y, row, width, height);
        int32_t *far_line = kFar ? box_line(far, box_off, bb, blockIdx.y, row, width, height) : nullptr;
        for (int x = bb.x + (int)lane; x <= bb.z; x += 64) { line[x] = INT_MAX; if constexpr (kFar) far_line[x] = INT_MIN; }
    }
}
__global__ __launch_bounds__(256) void fill_box_kernel(int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                       const uint32_t *__restrict__ box_off)
{
    fill_box_rows<false>(depth, nullptr, bbox, width, height, box_off);
}
__global__ __launch_bounds__(256) void fill_span_box_kernel(int32_t *__restrict__ depth, int32_t *__restrict__ far, const int4 *__restrict__ bbox,
                                                            uint32_t width, uint32_t height, const uint32_t *__restrict__ box_off)
{
    fill_box_rows<true>(depth, far, bbox, width, height, box_off);
}
__global__ __launch_bounds__(256) void count_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width,
                                                        uint32_t height, uint32_t *__restrict__ row_count, const uint32_t *__restrict__ box_off)
{
    // latency-bound, not bandwidth-bound: every lane keeps 4 rows x 4 column chunks = 16 loads in flight before the first ballot
    const uint32_t lane = threadIdx.x & 63;
    const int4 bb = bbox[blockIdx.y];
    const uint32_t row0 = blockIdx.x * kBoxRowsPerBlock + (threadIdx.x >> 6) * 4;
    uint32_t cnt[4] = { 0, 0, 0, 0 };
    for (int x0 = bb.x; x0 <= bb.z; x0 += 256) {
        int32_t v[4][4];
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t row = row0 + r;
            const int ry = (int)height - 1 - (int)row;
            const bool live = row < height && ry >= bb.y && ry <= bb.w;
            const int32_t *line = live ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, row, width, height) : depth;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int x = x0 + 64 * j + (int)lane; v[r][j] = (live && x <= bb.z) ? line[x] : 0; }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt[r] += (uint32_t)__popcll(__ballot(v[r][j] > 0 && v[r][j] != INT_MAX));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) if (row0 + r < height) row_count[(size_t)blockIdx.y * height + row0 + r] = cnt[r];
    }
}

// The same two steps for BANDED boxes (pose_box.h, band_box; asynchronous fused path, option box_bands).  A box is one contiguous run of
// 4 * w * nb ints at a 128-byte aligned offset: the fill is linear, 16 bytes per store, no row addresses; the workgroups of a hypothesis stride
// over it.  Box and offset come from device memory, so tight boxes keep their saving.
__global__ __launch_bounds__(256) void fill_band_kernel(int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t height,
                                                        const uint32_t *__restrict__ box_off)
{
    const BandBox k = band_box(bbox[blockIdx.y], height);
    const uint32_t n4 = (uint32_t)k.w * k.nb;                       // 16-byte words: one column of one band each
    int4 *dst = reinterpret_cast<int4 *>(depth + box_off[blockIdx.y]);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) dst[i] = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
}
// Grid as count_box_kernel: 16 image rows per workgroup, four aligned rows per wavefront -- exactly one band.  A lane loads one 16-byte word (a
// column of the band, its four rows), four words in flight (the 16 values count_box_kernel keeps), one ballot per row.  Rows of the band outside
// the box hold the fill value and count 0, which is what row_count holds for them; so do the rows of a band the box does not reach.
__global__ __launch_bounds__(256) void count_band_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t height,
                                                         uint32_t *__restrict__ row_count, const uint32_t *__restrict__ box_off)
{
    const uint32_t lane = threadIdx.x & 63;
    const BandBox k = band_box(bbox[blockIdx.y], height);
    const uint32_t row0 = blockIdx.x * kBoxRowsPerBlock + (threadIdx.x >> 6) * 4;
    if (row0 >= height) return;
    const uint32_t band = (row0 >> 2) - (uint32_t)(k.R >> 2);       // (wraps for a band above the box: not live)
    uint32_t cnt[4] = { 0, 0, 0, 0 };
    if (k.nb > 0 && row0 >= (uint32_t)k.R && band < k.nb) {
        const int4 *line = reinterpret_cast<const int4 *>(depth + box_off[blockIdx.y]) + (size_t)band * (uint32_t)k.w;
        for (int c0 = 0; c0 < k.w; c0 += 256) {
            int4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = line[min(c0 + 64 * j + (int)lane, k.w - 1)];      // (a lane past the end re-reads the last column: unconditional loads stay in flight together)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = c0 + 64 * j + (int)lane < k.w;
                cnt[0] += (uint32_t)__popcll(__ballot(in && v[j].x > 0 && v[j].x != INT_MAX));
                cnt[1] += (uint32_t)__popcll(__ballot(in && v[j].y > 0 && v[j].y != INT_MAX));
                cnt[2] += (uint32_t)__popcll(__ballot(in && v[j].z > 0 && v[j].z != INT_MAX));
                cnt[3] += (uint32_t)__popcll(__ballot(in && v[j].w > 0 && v[j].w != INT_MAX));
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) if (row0 + r < height) row_count[(size_t)blockIdx.y * height + row0 + r] = cnt[r];
    }
}

// Persistent workgroups walk the (hypothesis, band) items; a band is a run of raster rows of the
// hypothesis' box that fits the LDS tile.  Each workgroup rasterises ALL triangles against its band
// with ds_min, then writes the band (INT_MAX = empty) and its per-row valid counts.
__global__ __launch_bounds__(1024) void raster_band_kernel(const pr_triangle *__restrict__ tris, uint32_t n_tris,
                                                           const pr_mat4 *__restrict__ poses, uint32_t n_poses,
                                                           const int4 *__restrict__ bbox, int32_t *__restrict__ depth,
                                                           uint32_t *__restrict__ row_count, uint32_t width, uint32_t height,
                                                           pr_mat4 proj, uint32_t cap_px, uint32_t max_bands)
{
    extern __shared__ __attribute__((aligned(16))) int32_t tile[];
    const uint32_t n_items = n_poses * max_bands;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t pose = item / max_bands, band = item - pose * max_bands;
        const int4 bb = bbox[pose];
        const int bw = bb.z - bb.x + 1, bh = bb.w - bb.y + 1;
        if (bw <= 0 || bh <= 0) continue;
        const int rows_per_band = max(1, (int)(cap_px / (uint32_t)bw));
        const int n_bands = (bh + rows_per_band - 1) / rows_per_band;
        if ((int)band >= n_bands) continue;
        const int by0 = bb.y + (int)band * rows_per_band;
        const int by1 = min(bb.w, by0 + rows_per_band - 1);
        const int n_px = (by1 - by0 + 1) * bw;
        for (int i = threadIdx.x; i < n_px; i += 1024) tile[i] = INT_MAX;
        __syncthreads();

        const float *M = poses[pose].m;
        const float cmin0 = (float)bb.x, cmax0 = (float)bb.z, cmin1 = (float)by0, cmax1 = (float)by1;
        for (uint32_t ti = threadIdx.x; ti < n_tris; ti += 1024) {
            const float *tv = reinterpret_cast<const float *>(tris + ti);
            float px[3], py[3], w3[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = tv[3 * k], y = tv[3 * k + 1], z = tv[3 * k + 2];
                const float lx = M[0] * x + M[1] * y + M[2] * z + M[3];
                const float ly = M[4] * x + M[5] * y + M[6] * z + M[7];
                const float lz = M[8] * x + M[9] * y + M[10] * z + M[11];
                w3[k] = lz;
                const float cxp = proj.m[0] * lx + proj.m[1] * ly + proj.m[2] * lz + proj.m[3];
                const float cyp = proj.m[4] * lx + proj.m[5] * ly + proj.m[6] * lz + proj.m[7];
                px[k] = cxp / lz * (float)width / 2.0f + (float)width / 2.0f;
                py[k] = cyp / lz * (float)height / 2.0f + (float)height / 2.0f;
            }
            float lo0 = FLT_MAX, lo1 = FLT_MAX, hi0 = -FLT_MAX, hi1 = -FLT_MAX;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo0 = sel_max(cmin0, sel_min(lo0, px[k]));  hi0 = sel_min(cmax0, sel_max(hi0, px[k]));
                lo1 = sel_max(cmin1, sel_min(lo1, py[k]));  hi1 = sel_min(cmax1, sel_max(hi1, py[k]));
            }
            const float area = area2(px[0], py[0], px[1], py[1], px[2], py[2]);
            if (!(area != 0.0f)) continue;
            const float base_inv = 1 / area;
            const int x0 = loop_start(lo0 + 0.5f);
            for (int y = loop_start(lo1 + 0.5f); (float)y <= hi1; ++y) {
                const float fy = (float)y;
                for (int x = x0; (float)x <= hi0; ++x) {
                    const float fx = (float)x;
                    const float beta  = area2(px[0], py[0], fx, fy, px[2], py[2]) * base_inv;
                    const float gamma = area2(px[0], py[0], px[1], py[1], fx, fy) * base_inv;
                    const float alpha = 1.0f - beta - gamma;
                    if (alpha < -0.0f || beta < -0.0f || gamma < -0.0f || alpha > 1.0f || beta > 1.0f || gamma > 1.0f) continue;
                    const float az = alpha / w3[0], bz = beta / w3[1], gz = gamma / w3[2];
                    const float frag = (alpha + beta + gamma) / (az + bz + gz);
                    atomicMin(&tile[(y - by0) * bw + (x - bb.x)], f2i_x86(frag + 0.5f));
                }
            }
        }
        __syncthreads();

        // write the band: raster row y lands on image row height-1-y (renderer.cu:142)
        int32_t *img = depth + (size_t)pose * width * height;
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int r = (int)wave; r <= by1 - by0; r += 16) {
            const int yw = (int)height - 1 - (by0 + r);
            uint32_t cnt = 0;
            for (int c0 = 0; c0 < bw; c0 += 64) {
                const int c = c0 + (int)lane;
                int32_t v = INT_MAX;
                if (c < bw) { v = tile[r * bw + c]; img[(size_t)yw * width + bb.x + c] = v; }
                cnt += (uint32_t)__popcll(__ballot(c < bw && v > 0 && v != INT_MAX));
            }
            if (lane == 0) row_count[(size_t)pose * height + yw] = cnt;
        }
        __syncthreads();
    }
}

hipError_t launch_fill_i32(int32_t *dst, size_t n, int32_t v, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(cap_grid((n + 1023) / 1024)), dim3(256), 0, s, dst, n, v);
    return hipGetLastError();
}

hipError_t launch_sentinel2zero(int32_t *plane, size_t n, bool far, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    auto *kernel = far ? max2zero_kernel<INT_MIN> : max2zero_kernel<INT_MAX>;
    hipLaunchKernelGGL(kernel, dim3(cap_grid((n + 1023) / 1024)), dim3(256), 0, s, plane, n);
    return hipGetLastError();
}

// hypotheses a raster workgroup walks with its 256 triangles: 1 while the mesh is L2-resident and the grid is what fills the chip, more once
// the mesh has to be streamed (PR_RASTER_RUN overrides: experiments)
static uint32_t raster_pose_run(uint32_t n_tris, uint32_t n_poses)
{
    static const int env_run = getenv("PR_RASTER_RUN") ? atoi(getenv("PR_RASTER_RUN")) : 0;
    uint32_t run = 1;
    if (env_run > 0) run = (uint32_t)env_run;
    else if ((size_t)n_tris * sizeof(pr_triangle) > ((size_t)3 << 20)) run = 8;      // beyond what one XCD's 4 MiB L2 keeps next to the depth images
    if (run > n_poses) run = n_poses ? n_poses : 1u;
    return run;
}
// the groups the host filled (tris, n_tris, first, count), completed in place: empty groups dropped, run, triangle blocks, first workgroup; returns how many are left
static uint32_t complete_raster_groups(RasterGroup *groups_host, uint32_t n_groups, unsigned long long &total)
{
    uint32_t n = 0;
    total = 0;
    for (uint32_t i = 0; i < n_groups; ++i) {
        RasterGroup gr = groups_host[i];
        if (gr.n_tris == 0 || gr.count == 0) continue;             // an empty mesh renders nothing
        gr.run = raster_pose_run(gr.n_tris, gr.count);
        gr.tri_blocks = (gr.n_tris + 255) / 256;
        gr.first_wg = total;
        total += (unsigned long long)gr.tri_blocks * ((gr.count + gr.run - 1) / gr.run);
        groups_host[n++] = gr;
    }
    return n;
}
// the target as hypothesis p0 of it sees it: full frames follow one another, packed boxes keep the base and move on in their offsets
static RasterTarget target_at(RasterTarget t, uint32_t p0)
{
    const size_t first = t.box_off ? 0 : (size_t)p0 * t.rw * t.rh;
    t.depth += first;
    if (t.far) t.far += first;
    if (t.boxes) t.boxes += p0;
    if (t.box_off) t.box_off += p0;
    return t;
}
// Every raster launch but the LDS-band one.  One mesh: raster_kernel (raster_span_kernel with a far plane) over the hypotheses in runs of at most
// 32768, `check` riding on the first.  A mixed batch: the groups completed in the pinned block (complete_raster_groups), staged to groups_dev, and
// one raster_multi_kernel (raster_span_multi_kernel) launch over all of them.  An empty mesh launches nothing.
hipError_t launch_raster(const RasterMesh &mesh, const pr_mat4 *poses_dev, uint32_t n_poses, const RasterTarget &t, const BatchCheck *check, hipStream_t s)
{
    if (mesh.groups_host) {
        unsigned long long total = 0;
        const uint32_t n = complete_raster_groups(mesh.groups_host, mesh.n_groups, total);
        if (n == 0) return hipSuccess;
        hipError_t e = launch_stage_words(mesh.groups_mapped, mesh.groups_dev, sizeof(RasterGroup) * n, s);
        if (e != hipSuccess) return e;
        const dim3 grid((uint32_t)(total < (1ull << 22) ? total : (1ull << 22)));
        if (t.far)
            hipLaunchKernelGGL(raster_span_multi_kernel, grid, dim3(256), 0, s, (const RasterGroup *)mesh.groups_dev, n, total, poses_dev, t.depth, t.far,
                               t.width, t.height, *t.proj, t.roi, t.rw, t.rh, t.boxes, t.box_off);
        else
            hipLaunchKernelGGL(raster_multi_kernel, grid, dim3(256), 0, s, (const RasterGroup *)mesh.groups_dev, n, total, poses_dev, t.depth,
                               t.width, t.height, *t.proj, t.roi, t.rw, t.rh, t.boxes, t.box_off, t.image_of);
        return hipGetLastError();
    }
    if (mesh.n_tris == 0 || n_poses == 0) return hipSuccess;
    for_pose_launches(n_poses, [&](uint32_t p0, uint32_t np) {
        const RasterTarget u = target_at(t, p0);
        const uint32_t run = raster_pose_run(mesh.n_tris, np);
        const dim3 grid((mesh.n_tris + 255) / 256, (np + run - 1) / run);
        auto *kernel = u.bands ? raster_kernel<true> : raster_kernel<false>;
        if (u.far)
            hipLaunchKernelGGL(raster_span_kernel, grid, dim3(256), 0, s, mesh.tris, mesh.n_tris, poses_dev + p0, u.depth, u.far, u.width, u.height, *u.proj,
                               u.roi, u.rw, u.rh, u.boxes, np, run, u.box_off);
        else
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, mesh.tris, mesh.n_tris, poses_dev + p0, u.depth, u.width, u.height, *u.proj, u.roi, u.rw, u.rh,
                               u.boxes, np, run, u.box_off, (check && p0 == 0) ? *check : BatchCheck{});
        return hipSuccess;
    });
    return hipGetLastError();
}

// keys: 6 x uint32 scratch; aabb_out (device, 6 floats) and/or flag_out (device-visible word: 1 when the box differs from `expect`)
hipError_t launch_model_aabb(const pr_triangle *tris, uint32_t n_tris, uint32_t *keys, float *aabb_out, const float *expect, uint32_t *flag_out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(keys, 0xff, 6 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (n_tris > 0) {
        const uint32_t blocks = (n_tris * 3u + 2047u) / 2048u;           // >= 8 vertices per lane
        hipLaunchKernelGGL(model_aabb_kernel, dim3(blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks)), dim3(256), 0, s, tris, n_tris, keys);
    }
    AabbExpected ex{};
    if (expect) for (int a = 0; a < 6; ++a) ex.v[a] = expect[a];
    hipLaunchKernelGGL(model_aabb_finish_kernel, dim3(1), dim3(64), 0, s, keys, aabb_out, ex, flag_out);
    return hipGetLastError();
}

// fused-path render: boxes, LDS-band raster (depth + row counts), row scan.  Leaves depth valid only
// inside each hypothesis' box; row_count/row_off/counts as launch_depth2cloud(emit=false) would.
hipError_t launch_render_bands(const pr_triangle *tris, uint32_t n_tris, const pr_mat4 *poses_dev, uint32_t n_poses, const float *aabb,
                               int4 *bbox, int32_t *depth, uint32_t *row_count, uint32_t *row_off, uint32_t *counts,
                               uint32_t width, uint32_t height, const pr_mat4 &proj, pr_roi roi, uint32_t n_cus, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    const uint32_t cap_px = 36864;                                  // 144 KiB of the 160 KiB LDS
    if (!lds_opt_in(reinterpret_cast<const void *>(raster_band_kernel), 0, (uint32_t)(cap_px * sizeof(int32_t)))) return hipErrorInvalidValue;   // per device
    hipLaunchKernelGGL(pose_bbox_kernel, dim3((n_poses + 255) / 256), dim3(256), 0, s, aabb, poses_dev, n_poses, proj, width, height, roi, bbox);
    hipError_t e = hipMemsetAsync(row_count, 0, sizeof(uint32_t) * (size_t)n_poses * height, s);
    if (e != hipSuccess) return e;
    const uint32_t rows_min = cap_px / width > 0 ? cap_px / width : 1;
    const uint32_t max_bands = (height + rows_min - 1) / rows_min;
    const uint32_t items = n_poses * max_bands;
    const uint32_t grid = items < n_cus ? items : n_cus;
    hipLaunchKernelGGL(raster_band_kernel, dim3(grid), dim3(1024), cap_px * sizeof(int32_t), s, tris, n_tris, poses_dev, n_poses, bbox, depth,
                       row_count, width, height, proj, cap_px, max_bands);
    { hipError_t e = launch_d2c_scan(row_count, height, row_off, counts, n_poses, s); if (e != hipSuccess) return e; }
    return hipGetLastError();
}

// offsets of the packed boxes from boxes computed on the device (synchronous path; the asynchronous path's host computes both): exclusive scan of
// the areas rounded up to kBoxPack pixels (box_slot), one workgroup
__global__ __launch_bounds__(256) void box_pack_offsets_kernel(const int4 *__restrict__ bbox, uint32_t n, uint32_t *__restrict__ off, uint32_t height, bool bands)
{
    __shared__ uint32_t buf[256];
    __shared__ uint32_t carry;
    block_exclusive_scan(n, buf, &carry, [&](uint32_t i) { return box_slot_of(bbox[i], height, bands); }, [&](uint32_t i, uint32_t o) { off[i] = o; });
}
// the offsets of the packed boxes (nothing to do when the boxes lie in full frames)
static void launch_box_pack(const int4 *bbox, uint32_t n_poses, const uint32_t *box_off, hipStream_t s, uint32_t height = 0, bool bands = false)
{
    if (box_off) hipLaunchKernelGGL(box_pack_offsets_kernel, dim3(1), dim3(256), 0, s, bbox, n_poses, const_cast<uint32_t *>(box_off), height, bands);   // (the caller's scratch: filled here)
}
// Asynchronous path, option tight_box: the uploaded loose boxes of all n_poses hypotheses replaced by their tight ones ...
hipError_t launch_tight_boxes(const float4 *verts, uint32_t n_verts, const pr_mat4 *poses_dev, uint32_t n_poses, const pr_mat4 &proj,
                              uint32_t width, uint32_t height, int4 *bbox, hipStream_t s)
{
    if (n_poses == 0 || n_verts == 0) return hipSuccess;
    hipLaunchKernelGGL(pose_tight_box_kernel, dim3(n_poses), dim3(kTightLanes), 0, s, verts, n_verts, poses_dev, proj, width, height, bbox);
    return hipGetLastError();
}
// ... and the packed offsets of one sub-batch's boxes formed again from them (the uploaded ones belong to the loose boxes)
hipError_t launch_box_pack_offsets(const int4 *bbox, uint32_t n_poses, uint32_t *box_off, uint32_t height, bool bands, hipStream_t s)
{
    if (n_poses > 0) launch_box_pack(bbox, n_poses, box_off, s, height, bands);
    return hipGetLastError();
}
// the boxes of the first n hypotheses of `t` filled with "nothing drawn" (with a far plane: both planes), and their valid pixels counted row by row
static void launch_fill_boxes(const RasterTarget &t, uint32_t n, hipStream_t s)
{
    for_pose_launches(n, [&](uint32_t p0, uint32_t np) {
        const RasterTarget u = target_at(t, p0);
        const dim3 grid((u.height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np);
        if (u.bands) hipLaunchKernelGGL(fill_band_kernel, grid, dim3(256), 0, s, u.depth, u.boxes, u.height, u.box_off);
        else if (u.far) hipLaunchKernelGGL(fill_span_box_kernel, grid, dim3(256), 0, s, u.depth, u.far, u.boxes, u.width, u.height, u.box_off);
        else hipLaunchKernelGGL(fill_box_kernel, grid, dim3(256), 0, s, u.depth, u.boxes, u.width, u.height, u.box_off);
        return hipSuccess;
    });
}
static void launch_count_boxes(const RasterTarget &t, uint32_t n, uint32_t *row_count, hipStream_t s)
{
    for_pose_launches(n, [&](uint32_t p0, uint32_t np) {
        const RasterTarget u = target_at(t, p0);
        const dim3 grid((u.height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np);
        uint32_t *rows = row_count + (size_t)p0 * u.height;
        if (u.bands) hipLaunchKernelGGL(count_band_kernel, grid, dim3(256), 0, s, (const int32_t *)u.depth, u.boxes, u.height, rows, u.box_off);
        else hipLaunchKernelGGL(count_box_kernel, grid, dim3(256), 0, s, (const int32_t *)u.depth, u.boxes, u.width, u.height, rows, u.box_off);
        return hipSuccess;
    });
}

// Fused-path render, reference scheme (global int32 atomicMin) but only inside each hypothesis' box: the pixel boxes (compute_boxes: from mesh.aabb under
// t.roi -- hypothesis p takes the box of mesh mesh.box_index[p] when an index is given -- and, packed, their offsets; otherwise the caller placed both),
// the fill, the raster (launch_raster; a ROI is already part of the boxes), and -- rows.row_count given -- the row counts and the closing row scan
// (launch_d2c_scan_init when the asynchronous path's per-hypothesis records are given).  One mesh: fill, raster and count per run of 32768 hypotheses.
// With t.far both planes are filled and rastered (row-major boxes).  t.boxes, t.rw and t.rh are set here.
hipError_t launch_render_boxes(const RasterMesh &mesh, const pr_mat4 *poses_dev, uint32_t n_poses, int4 *bbox, const RasterTarget &target, const BoxRows &rows,
                               hipStream_t s, bool compute_boxes, const BatchCheck *check)
{
    if (n_poses == 0) return hipSuccess;
    if (target.bands && (!target.box_off || compute_boxes || target.far)) return hipErrorInvalidValue;      // banded boxes are packed boxes the caller placed (box_slot_of)
    RasterTarget t = target;
    t.boxes = bbox; t.rw = t.width; t.rh = t.height; t.roi = pr_roi{ 0, 0, 0, 0 };
    if (compute_boxes) {
        const dim3 grid((n_poses + 255) / 256);
        if (mesh.box_index) hipLaunchKernelGGL(pose_bbox_multi_kernel, grid, dim3(256), 0, s, mesh.aabb, mesh.box_index, poses_dev, n_poses, *t.proj, t.width, t.height, target.roi, bbox);
        else hipLaunchKernelGGL(pose_bbox_kernel, grid, dim3(256), 0, s, mesh.aabb, poses_dev, n_poses, *t.proj, t.width, t.height, target.roi, bbox);
        launch_box_pack(bbox, n_poses, t.box_off, s);
    }
    auto pass = [&](uint32_t p0, uint32_t np) {
        const RasterTarget u = target_at(t, p0);
        launch_fill_boxes(u, np, s);
        const hipError_t e = launch_raster(mesh, poses_dev + p0, np, u, p0 == 0 ? check : nullptr, s);
        if (e == hipSuccess && rows.row_count) launch_count_boxes(u, np, rows.row_count + (size_t)p0 * t.height, s);
        return e;
    };
    hipError_t e = mesh.groups_host ? pass(0, n_poses) : for_pose_launches(n_poses, pass);      // (a mixed batch's raster is one launch over all its groups)
    if (e != hipSuccess || !rows.row_count) return e != hipSuccess ? e : hipGetLastError();
    e = rows.meta ? launch_d2c_scan_init(rows.row_count, t.height, rows.row_off, rows.counts, n_poses, rows.meta, rows.st, rows.arrive, s)
                  : launch_d2c_scan(rows.row_count, t.height, rows.row_off, rows.counts, n_poses, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// ---- mixed batches (hypotheses of several meshes in one call) -----------------------------------------------------------------------
hipError_t launch_model_aabb_multi(const pr_mesh_ref *meshes_dev, const pr_mesh_ref *meshes_host, uint32_t n_meshes, uint32_t *keys, float *aabb_out, hipStream_t s)
{
    if (n_meshes == 0) return hipSuccess;
    hipError_t e = launch_fill_i32(reinterpret_cast<int32_t *>(keys), 6 * (size_t)n_meshes, -1, s);     // all ones: no copy or fill command
    if (e != hipSuccess) return e;
    uint32_t most = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) if ((uint32_t)meshes_host[m].n_tris > most) most = (uint32_t)meshes_host[m].n_tris;
    if (most > 0) {
        const uint32_t blocks = (most * 3u + 2047u) / 2048u;               // as launch_model_aabb, sized by the largest mesh
        hipLaunchKernelGGL(model_aabb_multi_kernel, dim3(blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks), n_meshes < 65535 ? n_meshes : 65535), dim3(256), 0, s,
                           meshes_dev, n_meshes, keys);
    }
    const uint32_t words = 6 * n_meshes;
    hipLaunchKernelGGL(model_aabb_multi_finish_kernel, dim3((words + 255) / 256), dim3(256), 0, s, keys, words, aabb_out);
    return hipGetLastError();
}

}  // namespace prk
