// contour_fit.h -- what contour_fit.hip (the silhouette's normal equations) shares with score_core (pr_refine.cpp)
#pragma once
#include "pr_internal.h"

namespace prk {

constexpr uint32_t kFitSums = 28;                                  // H[21], g[6], the sum of res^2 (sum_wr2 and sum_r2 are both it; sum_w = 2 * used)

// one hypothesis of a launch: its centre (camera frame, metres) and radius; and what every hypothesis shares: K[0], K[2], K[4], K[5], each
// converted to double once, tau_mm and jump_mm
struct alignas(16) FitMeta { float c[3], rho; };
static_assert(sizeof(FitMeta) == 16, "FitMeta: one 16-byte word");
struct FitParams { double fx, cx, fy, cy; int32_t tau, jump; };
constexpr uint32_t kFitRowsPerBlock = 16;                          // kBoxRowsPerBlock (pr_device.h), for the host: image rows per workgroup
inline uint32_t fit_blocks(uint32_t height) { return (height + kFitRowsPerBlock - 1) / kFitRowsPerBlock; }      // partial sums per hypothesis

// partial: [n_poses][fit_blocks(height)][kFitSums] doubles of scratch; records[8 * i]: pr_contour_fit words (contour, used, occluded,
// miss, reserved x 2, sum_d2 lo / hi), which the caller zeroed; info[n_poses]: written whole by the second launch.  window as for launch_contour_boxes
hipError_t launch_contour_fit(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                              const void *scene, bool scene_i32, const uint32_t *nearest, const FitMeta *meta, const FitParams &pm, uint32_t *records,
                              double *partial, pr_pose_info *info, hipStream_t s);

}  // namespace prk
