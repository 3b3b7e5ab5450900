// Training targets of the CenterNet loss (reference loss.py:31-135), gfx950.
//
// The reference loops over samples and objects in Python and, per object, evaluates a Gaussian
// over the whole output map (out_h x out_w exp per object) and takes an elementwise max into
// the object's plane. Here one thread owns one cell of one (sample, plane) and walks that
// sample's objects in the reference's order, so every cell's value is the same sequence of
// fp32 operations the reference applies to it:
//   center cell   floor(fl32(fl32(c * in) / ratio))                       (loss.py:52-53, 103-104)
//   Gaussian      exp(fl32(-d2) / fl32(2 sigma^2)), d2 exact integer      (:64-67, 106-114)
//   max           torch.maximum (NaN propagates), nan_to_num at the end   (:70, 131-133)
//   affinity      unit displacement from the owning object's center to the cell, taken where
//                 its length is strictly below the running minimum: the earliest instance
//                 wins ties (:116-129)
// Output planes are written once, coalesced (consecutive threads = consecutive cells). The
// reference's exp is torch's CPU expf; this is the device expf (both ~1 ulp). The affinity's
// sqrt and quotient are correctly rounded here; torch's CPU sqrt (MKL VML vsSqrt) returns one
// ulp below the correctly rounded root for ~0.6% of fp32 inputs (tests/test_targets.py).
// The per-cell functions live in targets_dev.h, which the loss kernels (loss.hip) share.
#include "targets_dev.h"

namespace tv {
namespace targets {

// heatmap [B][L][H][W]: grid (cells / 256, L, B)
__global__ __launch_bounds__(256) void heatmap(const Truth t, int L, float den, float* __restrict__ out) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int l = blockIdx.y, b = blockIdx.z;
  if (q >= t.H * t.W) return;
  const int y = q / t.W, x = q - y * t.W;
  out[((size_t)b * L + l) * t.H * t.W + q] = heat_cell(t, b, l, y, x, den);
}

// keypoint heatmap / affinity weight [B][K][H][W], affinity [B][K][2][H][W]: grid (cells / 256, K, B)
__global__ __launch_bounds__(256) void keypoints(const Truth t, int K, float den_h, float den_a,
                                                  float* __restrict__ heat, float* __restrict__ aw,
                                                  float* __restrict__ aff) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, b = blockIdx.z;
  const int H = t.H, W = t.W;
  if (q >= H * W) return;
  const int y = q / W, x = q - y * W;
  const KeypointCell c = keypoint_cell(t, b, k, y, x, den_h, den_a);
  const size_t plane = (size_t)b * K + k;
  heat[plane * H * W + q] = c.heat;
  aw[plane * H * W + q] = c.weight;
  aff[(2 * plane) * H * W + q] = c.a0;
  aff[(2 * plane + 1) * H * W + q] = c.a1;
}

}  // namespace targets

int launch_train_heatmap(const uint8_t* valid, const long long* label, const float* center, int B, int n_obj, int L,
                         int in_h, int in_w, int ratio, double sigma, float* out, hipStream_t s) {
  if (B < 1 || n_obj < 0 || L < 1 || in_h < 1 || in_w < 1 || ratio < 1 || !out || (n_obj && (!valid || !label || !center))) {
    set_error("generate_heatmap: bad arguments");
    return 1;
  }
  const int H = in_h / ratio, W = in_w / ratio;
  if (H < 1 || W < 1) {
    set_error("generate_heatmap: empty output map");
    return 2;
  }
  if (sigma < 0.1) sigma = 0.1;  // loss.py:59-63
  targets::Truth t{};
  t.valid = valid; t.label = label; t.center = center; t.n_obj = n_obj;
  t.in_h = in_h; t.in_w = in_w; t.ratio = ratio; t.H = H; t.W = W;
  hipLaunchKernelGGL(targets::heatmap, dim3((H * W + 255) / 256, L, B), dim3(256), 0, s, t, L, targets::den_of(sigma),
                     out);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_train_keypoints(const uint8_t* kvalid, const long long* klabel, const float* kcenter, const long long* kobj,
                           const float* center, int B, int n_inst, int n_obj, int K, int in_h, int in_w, int ratio,
                           double heat_sigma, double aff_sigma, float* heat, float* aw, float* aff, hipStream_t s) {
  if (B < 1 || n_inst < 0 || n_obj < 0 || K < 1 || in_h < 1 || in_w < 1 || ratio < 1 || !heat || !aw || !aff ||
      (n_inst && (!kvalid || !klabel || !kcenter || !kobj || !center))) {
    set_error("generate_keypoint_heatmap: bad arguments");
    return 1;
  }
  const int H = in_h / ratio, W = in_w / ratio;
  if (H < 1 || W < 1) {
    set_error("generate_keypoint_heatmap: empty output map");
    return 2;
  }
  targets::Truth t{};
  t.kvalid = kvalid; t.klabel = klabel; t.kcenter = kcenter; t.kobj = kobj; t.center = center;
  t.n_inst = n_inst; t.n_obj = n_obj;
  t.in_h = in_h; t.in_w = in_w; t.ratio = ratio; t.H = H; t.W = W;
  hipLaunchKernelGGL(targets::keypoints, dim3((H * W + 255) / 256, K, B), dim3(256), 0, s, t, K,
                     targets::den_of(heat_sigma), targets::den_of(aff_sigma), heat, aw, aff);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
