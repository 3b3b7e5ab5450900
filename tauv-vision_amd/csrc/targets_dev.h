// Device functions of the CenterNet training targets (reference loss.py:31-135), shared by the kernels
// that store the target planes (targets.hip) and the loss kernels that consume each cell's target
// value on the fly (loss.hip): one definition, so both see the same fp32 operation sequence and the
// same object walk.
//   center cell   floor(fl32(fl32(c * in) / ratio))                       (loss.py:52-53, 103-104)
//   Gaussian      exp(fl32(-d2) / fl32(2 sigma^2)), d2 exact integer      (:64-67, 106-114)
//   max           torch.maximum (NaN propagates), nan_to_num at the end   (:70, 131-133)
//   affinity      unit displacement from the owning object's center to the cell, taken where
//                 its length is strictly below the running minimum: the earliest instance
//                 wins ties (:116-129)
#pragma once
#include "common.h"

#include <cfloat>
#include <cmath>

namespace tv {
namespace targets {

__device__ __forceinline__ float maximum_nan(float a, float b) {  // torch.maximum
  return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b);
}
__device__ __forceinline__ float nan_to_num(float v, float nan) {  // torch.nan_to_num(v, nan)
  return v != v ? nan : v == INFINITY ? FLT_MAX : v == -INFINITY ? -FLT_MAX : v;
}
__device__ __forceinline__ int cell(float c, int in_size, int ratio) {
  return (int)floorf(__fdiv_rn(__fmul_rn(c, (float)in_size), (float)ratio));
}
__device__ __forceinline__ float gauss(int x, int y, int cx, int cy, float den) {
  const long long dx = (long long)x - cx, dy = (long long)y - cy;
  const float d2 = (float)(dx * dx + dy * dy);
  return expf(__fdiv_rn(-d2, den));
}

// The truth tensors of one batch and the target grid (device pointers; the label / index tensors
// hold values already wrapped into [0, planes)).
struct Truth {
  const uint8_t* valid;      // [B][n_obj]
  const long long* label;    // [B][n_obj]
  const float* center;       // [B][n_obj][2]
  const uint8_t* kvalid;     // [B][n_inst]
  const long long* klabel;   // [B][n_inst]
  const float* kcenter;      // [B][n_inst][2]
  const long long* kobj;     // [B][n_inst]
  int n_obj, n_inst;
  int in_h, in_w, ratio, H, W;
};

// generate_heatmap's value of cell (y, x) of plane l of sample b (loss.py:46-70)
__device__ __forceinline__ float heat_cell(const Truth& t, int b, int l, int y, int x, float den) {
  float v = 0.f;
  for (int o = 0; o < t.n_obj; ++o) {
    const size_t bo = (size_t)b * t.n_obj + o;
    if (!t.valid[bo] || t.label[bo] != l) continue;
    const int cy = cell(t.center[2 * bo], t.in_h, t.ratio), cx = cell(t.center[2 * bo + 1], t.in_w, t.ratio);
    v = maximum_nan(v, gauss(x, y, cx, cy, den));
  }
  return nan_to_num(v, 0.f);
}

struct KeypointCell {
  float heat, weight, a0, a1;  // keypoint heatmap, affinity weight, affinity (y, x)
};

// generate_keypoint_heatmap's values of cell (y, x) of keypoint plane k of sample b (loss.py:94-133)
__device__ __forceinline__ KeypointCell keypoint_cell(const Truth& t, int b, int k, int y, int x, float den_h,
                                                      float den_a) {
  // the cell's normalised position, as torch.stack((y / out_h, x / out_w)) forms it
  const float py = __fdiv_rn((float)y, (float)t.H), px = __fdiv_rn((float)x, (float)t.W);
  float vh = 0.f, va = 0.f, a0 = 0.f, a1 = 0.f, dist = INFINITY;
  for (int i = 0; i < t.n_inst; ++i) {
    const size_t bi = (size_t)b * t.n_inst + i;
    if (!t.kvalid[bi] || t.klabel[bi] != k) continue;
    const int cy = cell(t.kcenter[2 * bi], t.in_h, t.ratio), cx = cell(t.kcenter[2 * bi + 1], t.in_w, t.ratio);
    vh = maximum_nan(vh, gauss(x, y, cx, cy, den_h));
    va = maximum_nan(va, gauss(x, y, cx, cy, den_a));
    const size_t bo = (size_t)b * t.n_obj + (size_t)t.kobj[bi];
    const float d0 = nan_to_num(__fsub_rn(py, t.center[2 * bo]), 0.f);
    const float d1 = nan_to_num(__fsub_rn(px, t.center[2 * bo + 1]), 0.f);
    const float dd = nan_to_num(__fsqrt_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1))), 1.f);
    if (dd < dist) {
      a0 = __fdiv_rn(d0, dd);
      a1 = __fdiv_rn(d1, dd);
    }
    dist = fminf(dist, dd);  // dd is never NaN here
  }
  return KeypointCell{nan_to_num(vh, 0.f), nan_to_num(va, 0.f), nan_to_num(a0, 0.f), nan_to_num(a1, 0.f)};
}

// fl32(2 sigma^2) with sigma^2 in double, as the Python expression `2 * sigma ** 2` hands it to torch
inline float den_of(double sigma) { return (float)(2.0 * (sigma * sigma)); }

}  // namespace targets
}  // namespace tv
