// Device arithmetic of torch's F.interpolate that more than one kernel restates: the source index
// and weights of mode="bilinear" (align_corners=False), the source index of mode="nearest", and the
// destination rows / columns that can map into a box crop of the source (localize.hip's
// bound_by_box, yolact_frame.hip's wave skip). Defined once so that the kernels cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace tv {
namespace resample {

// The taps and weights of a bilinear source position `src` on an axis of `in` pixels, as torch's
// upsample_bilinear2d clamps them (align_corners=False): src = max(0, src), i0 = floor (never past in - 1),
// the second tap clamped to in - 1, l1 = src - i0, l0 = 1 - l1. Both taps always lie inside the frame.
// augment.hip calls it with a homography's source position.
__device__ __forceinline__ void lin_taps(float src, int in, int& i0, int& i1, float& l0, float& l1) {
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
  l0 = __fsub_rn(1.f, l1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// torch's upsample_bilinear2d source index and weights, align_corners=False, scale = in / out in
// fp32 (area_pixel_compute_source_index): src = fma(scale, d + 0.5, -0.5), then lin_taps
__device__ __forceinline__ void lin_index(int d, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  lin_taps(__fmaf_rn(scale, (float)d + 0.5f, -0.5f), in, i0, i1, l0, l1);
}

// the blend of the four taps as torch's CPU kernel evaluates it: the row blend fma(top, h0, bottom * h1)
// of the column blends fma(left, w0, right * w1)
__device__ __forceinline__ float lin_blend(float tl, float tr, float bl, float br, float h0, float h1, float w0,
                                           float w1) {
  const float t0 = __fmaf_rn(tl, w0, __fmul_rn(tr, w1));
  const float t1 = __fmaf_rn(bl, w0, __fmul_rn(br, w1));
  return __fmaf_rn(t0, h0, __fmul_rn(t1, h1));
}

// torch's CPU nearest F.interpolate: src = min((int)floorf(dst * scale), n - 1), scale = (float)n / (float)dn
__device__ __forceinline__ int nearest_src(int dst, float scale, int n) {
  return min((int)floorf(__fmul_rn((float)dst, scale)), n - 1);
}

// The destination rows or columns (of dn) whose nearest source pixel can lie inside [lo, hi] of an
// n-pixel source axis (lo, hi: the box crop's bounds at mask resolution, as assemble_mask forms them).
// The range is widened on purpose — one source pixel for the rounding of the bounds, then two
// destination pixels (and dn / 2^18 for fp32 index arithmetic on very large images) for the rounding
// of the nearest map — because the mask is zero outside the crop: scanning more never changes the
// result. A bilinear tap pair (i0, i0 + 1) reaches one source pixel further than the nearest map on
// either side: such a caller passes lo - 1, hi + 1.
__device__ inline void crop_range(float lo, float hi, int n, int dn, int& d0, int& d1) {
  d0 = 0;
  d1 = dn - 1;
  if (!isfinite(lo) || !isfinite(hi)) return;
  const double l = fmin(fmax((double)lo, -1.0), (double)n), r = fmin(fmax((double)hi, -1.0), (double)n);
  const int sl = (int)floor(l) - 1, sr = (int)ceil(r) + 1;
  const int margin = 2 + (dn >> 18);
  const double f = (double)dn / (double)n;
  const double a = floor((double)sl * f) - margin, b = ceil((double)(sr + 1) * f) + margin;
  d0 = (int)fmin(fmax(a, 0.0), (double)dn);       // dn: empty
  d1 = (int)fmin(fmax(b, -1.0), (double)(dn - 1));
}

// crop_range on both axes for the box q = (y, x, h, w) of an mh x mw mask resized to dh x dw:
// box_to_mask (boxes.py:88-103) at mask resolution, the fp32 bounds of assemble_mask, each widened by
// `reach` source pixels (0 for the nearest map, 1 for bilinear)
__device__ inline void box_crop(const float* q, int mh, int mw, int dh, int dw, float reach, int& x0, int& x1, int& y0,
                                int& y1) {
#pragma clang fp contract(off)
  const float by = q[0] * (float)mh, bx = q[1] * (float)mw, bh = q[2] * (float)mh, bw = q[3] * (float)mw;
  crop_range(bx - bw / 2 - reach, bx + bw / 2 + reach, mw, dw, x0, x1);
  crop_range(by - bh / 2 - reach, by + bh / 2 + reach, mh, dh, y0, y1);
}

}  // namespace resample
}  // namespace tv
