// pr_device.h -- device-side helpers shared by every kernel file: x86 float->int semantics, offset loads, DPP lane access
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <float.h>
#include <stdlib.h>
#include <atomic>

#include "pr_internal.h"
#include "pr_tuning.h"

namespace prk {

// ------------------------------------------------------------------------------------------------
// conversions with the semantics the reference CPU build has on x86-64 (cvttss2si): out-of-range
// and NaN inputs give INT_MIN.  v_cvt_i32_f32 saturates instead, so the range test is explicit.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int f2i_x86(float v)
{
    return (v > -2147483904.0f && v < 2147483648.0f) ? (int)v : INT_MIN;
}
// size_t(float) for loop starts that are later compared against a bound < 2^24: anything
// outside (-1, 2^24) can never satisfy "(float)p <= bound", so it maps to "no iterations".
__device__ __forceinline__ int loop_start(float v)
{
    return (v > -1.0f && v < 16777216.0f) ? (int)v : INT_MAX;
}

__device__ __forceinline__ float sel_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float sel_min(float a, float b) { return (a < b) ? a : b; }

// One-instruction square root / reciprocal (v_sqrt_f32 / v_rcp_f32: 1 ulp) for SAFETY MARGINS only -- step lengths, window radii, slack: every
// use multiplies the result by a factor at least 1e-6 away from 1 on the safe side.  Never for a value the oracle is compared with bit by bit
// (sqrtf and '/' expand to the correctly rounded sequences there: ten instructions and more each).
__device__ __forceinline__ float margin_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }
__device__ __forceinline__ float margin_rcp(float v) { return __builtin_amdgcn_rcpf(v); }

typedef float float2v __attribute__((ext_vector_type(2)));
// base + 32-bit byte offset: lets the compiler address with a scalar base and one 32-bit VGPR (global_load ... v_off, s[base])
// instead of building a 64-bit address per lane (v_lshl_add_u64 / v_mad_u64_u32 plus the copies that come with 64-bit values)
template <class T> __device__ __forceinline__ T ld_off(const void *base, uint32_t byte_off)
{ return *reinterpret_cast<const T *>(static_cast<const char *>(base) + byte_off); }
template <class T> __device__ __forceinline__ void st_off(void *base, uint32_t byte_off, const T &v)
{ *reinterpret_cast<T *>(static_cast<char *>(base) + byte_off) = v; }
struct Corr { float dx, dy, dz, nx, ny, nz; };   // destination point and its normal

// ------------------------------------------------------------------------------------------------
// wave64 sum with a fixed balanced pairwise tree in lane order, result in lane 63:
//   row_shr:1,2,4,8 inside each 16-lane row, row_bcast15 into rows 1 and 3, row_bcast31 into rows 2,3.
// ------------------------------------------------------------------------------------------------
template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_get(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, kRowMask, 0xf, true));
}

// sampled fingerprint of up to three caller-owned arrays (scene_fingerprint_kernel, batch_check_kernel): this lane's share of the hash of a
// 256-lane workgroup -- 16 of the 4096 samples per array; the workgroup's fingerprint is the SUM of its lanes' values (order-free)
__device__ __forceinline__ uint32_t fingerprint_lane(const uint32_t *__restrict__ a, unsigned long long na, const uint32_t *__restrict__ b, unsigned long long nb,
                                                     const uint32_t *__restrict__ c, unsigned long long nc)
{
    uint32_t h = 0;
    const uint32_t *arr[3] = { a, b, c };
    const unsigned long long len[3] = { na, nb, nc };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!arr[k] || len[k] == 0) continue;
        // sample s of 4096 sits in stripe s of the array, at a hashed offset inside it (32-bit arithmetic: __umulhi maps a hash onto a range)
        const uint32_t n = len[k] > 0xffffffffull ? 0xffffffffu : (uint32_t)len[k];
        const uint32_t stripe = n / 4096u;                            // 0 for short arrays: every word is visited, wrapping around
        uint32_t w[16];
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint32_t s = threadIdx.x * 16u + i;
            const uint32_t pos = stripe ? s * stripe + __umulhi(s * 2654435761u + 0x9e3779b9u, stripe) : (n >= 4096u ? s : s % n);
            w[i] = arr[k][pos] ^ pos;
        }
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) h += w[i] * 2654435761u + (uint32_t)k;      // a sum: the order of the lanes does not matter
    }
    return h;
}

// wave64 sum of one uint32 per lane, the same value in every lane: in-row inclusive scan with DPP row shifts (lanes shifted in from outside
// the row read 0), then the four row totals by readlane (nn_search.hip's prefix sum, total only).  Integer adds: exact in any order.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);      // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);      // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);      // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);      // row_shr:8
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// Ordered compaction by one wavefront: THE count / emit loop of the frame stages (the PPF and plane samples, the segment roots, the kd-tree
// scene gather).  One step takes 64 items, a lane each: a kept lane's slot is base + the kept lanes below it, and the step's count moves the
// base on.  lane = the lane in its wavefront (a workgroup of several wavefronts runs one loop per wavefront); every lane takes every step.
struct WaveSlot { uint32_t pos, kept; };
__device__ __forceinline__ WaveSlot wave_compact_step(bool keep, uint32_t lane, uint32_t base)
{
    const unsigned long long m = __ballot(keep);
    return WaveSlot{ base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), (uint32_t)__popcll(m) };
}
// items 0 .. n-1 in ascending order, 64 at a time: the number keep(i) holds for, the same in every lane
template <class Keep>
__device__ __forceinline__ uint32_t wave_compact_count(uint32_t n, uint32_t lane, Keep &&keep)
{
    uint32_t total = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) total += wave_compact_step(i0 + lane < n && keep(i0 + lane), lane, 0).kept;
    return total;
}
// the same walk with the slots: visit(i, kept, pos) for every i < n (pos means something where kept); returns base + the number kept
template <class Keep, class Visit>
__device__ __forceinline__ uint32_t wave_compact_place(uint32_t n, uint32_t lane, uint32_t base, Keep &&keep, Visit &&visit)
{
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool kept = i < n && keep(i);
        const WaveSlot s = wave_compact_step(kept, lane, base);
        if (i < n) visit(i, kept, s.pos);
        base += s.kept;
    }
    return base;
}

// Exclusive scan of n values in chunks of 256 with a carry, by one 256-lane workgroup (Hillis-Steele per chunk): out(i, value(0) + ... + value(i - 1))
// for every i < n; returns the total in every lane.  THE scan of the render -> cloud stage: the row offsets of an image (d2c_scan_kernel,
// d2c_scan_init_kernel), the starts of the packed clouds (d2c_pack_starts_kernel), the offsets of the packed boxes (box_pack_offsets_kernel), the counts of a frame stage (scan_counts_kernel).
// buf: 256 words of LDS, carry: one more.
template <class Value, class Out>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t n, uint32_t *buf, uint32_t *carry, Value &&value, Out &&out)
{
    if (threadIdx.x == 0) *carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = (i < n) ? value(i) : 0u;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {           // Hillis-Steele inclusive scan
            const uint32_t t = (threadIdx.x >= off) ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) out(i, *carry + buf[threadIdx.x] - v);
        __syncthreads();
        if (threadIdx.x == 255) *carry += buf[255];
        __syncthreads();
    }
    return *carry;
}

constexpr uint32_t kBoxRowsPerBlock = 16;                        // rows of a pixel box per workgroup: 4 wavefronts x 4 rows (few, fatter workgroups: dispatch-bound otherwise)

// box_off (fused asynchronous path): the boxes of a sub-batch PACKED one behind the other, each as its own little image (pitch = its width) at
// box_off[hypothesis] ints -- like the clouds (d2c_pack_starts_kernel), and for the same reason: 290 KB boxes 1.2 MB apart make the render depend
// on the frame's size (a frame 17 or 32 rows taller: -3 %).  nullptr: full frames [hypothesis][height][width].
__device__ __forceinline__ int32_t *box_line(int32_t *depth, const uint32_t *box_off, const int4 bb, uint32_t pose, uint32_t row, uint32_t width, uint32_t height)
{
    if (!box_off) return depth + ((size_t)pose * height + row) * width;
    const ptrdiff_t pitch = max(bb.z - bb.x + 1, 0);
    return depth + box_off[pose] + ((ptrdiff_t)row - (ptrdiff_t)((int)height - 1 - bb.w)) * pitch - (ptrdiff_t)bb.x;      // line[x] for bb.x <= x <= bb.z
}

// depth2cloud's back-projection of frame pixel (x, row) with depth d in mm (icp.cu:249-253: z = d/1000.f; x = (u - cx)/fx*z; y = (v - cy)/fy*z):
// what every fused-path emit writes for a rendered pixel
__device__ __forceinline__ pr_vec3 backproject_pixel(int x, uint32_t row, int32_t d, float fx, float fy, float cx, float cy)
{
    const float z = d / 1000.0f;
    pr_vec3 p;
    p.x = ((float)(uint32_t)x - cx) / fx * z;
    p.y = ((float)row - cy) / fy * z;
    p.z = z;
    return p;
}
// transform_pcd (icp.cpp:47-59) of one point by rows 0..2 of a 4x4, in the fused pass' operand order: ((m0*x + m1*y) + m2*z) + m3
__device__ __forceinline__ pr_vec3 transform_point(const float *M, const pr_vec3 p)
{
    pr_vec3 q;
    q.x = M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3];
    q.y = M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7];
    q.z = M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11];
    return q;
}

}  // namespace prk
