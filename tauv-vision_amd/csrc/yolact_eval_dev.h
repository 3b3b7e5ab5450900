// The arithmetic of the YOLACT evaluation (yolact_eval.hip; contracts: tv_yolact_evaluate_match in
// include/tauv_vision_amd.h) that also compiles for the host (tools/yolact_eval_host_check.cpp): the two
// IoUs, the sortable score key, a detection's label and score from its softmax row. All in double on the
// fp32 / integer values, uncontracted, in the order written here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define TV_YE_HD __host__ __device__ __forceinline__

namespace tv {
namespace yeval {

// Box IoU of a detection and a truth given as centre (y, x) and size (h, w).
TV_YE_HD double box_iou(float dy, float dx, float dh, float dw, float ty, float tx, float th, float tw) {
#pragma clang fp contract(off)
  const double Yd = dy, Xd = dx, Hd = dh, Wd = dw, Yt = ty, Xt = tx, Ht = th, Wt = tw;
  const double y0d = Yd - Hd / 2, y1d = Yd + Hd / 2, x0d = Xd - Wd / 2, x1d = Xd + Wd / 2;
  const double y0t = Yt - Ht / 2, y1t = Yt + Ht / 2, x0t = Xt - Wt / 2, x1t = Xt + Wt / 2;
  const double ya = y0d > y0t ? y0d : y0t, yb = y1d < y1t ? y1d : y1t;
  const double xa = x0d > x0t ? x0d : x0t, xb = x1d < x1t ? x1d : x1t;
  double sy = yb - ya, sx = xb - xa;
  sy = sy > 0.0 ? sy : 0.0;
  sx = sx > 0.0 ? sx : 0.0;
  const double inter = sy * sx;
  const double a_d = Hd * Wd, a_t = Ht * Wt;
  const double den = a_d + a_t - inter;
  if (den <= 0.0) return 0.0;
  return inter / den;
}

// Mask IoU from the pixel counts.
TV_YE_HD double mask_iou(int inter, int det_area, int truth_area) {
  const long long uni = (long long)det_area + (long long)truth_area - (long long)inter;
  if (uni == 0) return 0.0;
  return (double)inter / (double)uni;
}

// A key that orders like the score: larger score, larger key; -0 == +0; NaN below everything.
TV_YE_HD unsigned score_key(float s) {
  if (s != s) return 0u;
  if (s == 0.0f) s = 0.0f;
  unsigned u;
  __builtin_memcpy(&u, &s, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Walks before: record j goes before record i.
TV_YE_HD bool walks_before(unsigned kj, int j, unsigned ki, int i) { return kj > ki || (kj == ki && j < i); }

// The label 1 + argmax over the foreground columns 1..C of a softmax row [C + 1] (a strict `>` scan
// from column 1: the lowest index on a tie; a NaN never replaces the running best) and its probability.
TV_YE_HD void label_score(const float* row, int C, int* label, float* score) {
  float best = row[1];
  int at = 1;
  for (int c = 2; c <= C; ++c)
    if (row[c] > best) { best = row[c]; at = c; }
  *label = at;
  *score = best;
}

}  // namespace yeval
}  // namespace tv
