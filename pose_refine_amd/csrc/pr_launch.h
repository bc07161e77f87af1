// pr_launch.h -- host-side helpers of the launchers (one copy per translation unit)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#pragma once
#include "pr_device.h"

namespace prk {

// Dynamic LDS beyond 64 KiB is an opt-in PER DEVICE (hipFuncSetAttribute applies to the current device): one flag per kernel slot and
// device, so that a process driving several GPUs (one host thread each) opts in on every one of them.
static bool lds_opt_in(const void *fn, int slot, uint32_t bytes)
{
    static std::atomic<uint64_t> done[8];                         // bit = device ordinal (<= 64 devices), one word per kernel slot
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done[slot].load(std::memory_order_acquire) & (1ull << dev)) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();                                 // a refusal is the caller's to handle (a smaller launch): it must not surface as that launch's error
        return false;
    }
    done[slot].fetch_or(1ull << dev, std::memory_order_release);
    return true;
}
static inline uint32_t cap_grid(size_t want) { return (uint32_t)(want < 1 ? 1 : (want > 8192 ? 8192 : want)); }
// fn(p0, np) over n hypotheses in runs of at most 32768 -- one per grid row, and grid.y is limited to 65535; ends at the first error
template <class Fn>
static inline hipError_t for_pose_launches(uint32_t n, Fn fn)
{
    for (uint32_t p0 = 0; p0 < n; p0 += 32768) {
        const hipError_t e = fn(p0, (n - p0 < 32768) ? (n - p0) : 32768u);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// fn(tag) with a null pointer of the depth image's element type, int32_t or uint16_t: a kernel template over that type is launched from one
// statement -- [&](auto *tag) { using T = std::remove_pointer_t<decltype(tag)>; ... kernel<T> ... static_cast<const T *>(depth) ... }
template <class Fn>
static inline void for_depth_type(bool depth_i32, Fn fn)
{
    if (depth_i32) fn(static_cast<int32_t *>(nullptr)); else fn(static_cast<uint16_t *>(nullptr));
}

// row scans of the depth -> cloud stage and the count scan of the frame stages (d2c.hip), called from the launchers of other files
hipError_t launch_scan_counts(uint32_t *counts, uint32_t n, uint32_t *offsets, uint32_t *total_out, bool clear, hipStream_t s);
hipError_t launch_d2c_scan(const uint32_t *row_count, uint32_t gh, uint32_t *row_off, uint32_t *counts, uint32_t n_img, hipStream_t s);
hipError_t launch_d2c_scan_init(const uint32_t *row_count, uint32_t gh, uint32_t *row_off, uint32_t *counts, uint32_t n_img,
                                PoseMeta *meta, DevIcpState *st, uint32_t *arrive, hipStream_t s);

}  // namespace prk
