// Depth localisation of detections: the per-detection loops of the two reference nodes that turn
// a detection into a camera-frame point from the raw mono16 depth image.
//   box mode   centernet_node.py:139-178  rectangle of +-0.4 w, +-0.4 h around the centre
//              (cv2.rectangle, filled), np.sum / np.mean of the positive depth inside it
//   mask mode  yolact_node.py:135,143,177-193  F.interpolate (nearest) of every assembled mask to
//              the raw image size, np.nanmean(np.where(mask > 0.5, depth, nan))
// One workgroup of 256 threads per (image, detection). Each wave takes every fourth row of the
// region, its lanes consecutive u16 pixels of the row: 16-byte loads (8 pixels) over the aligned
// body, single pixels over the unaligned head and tail (row starts are arbitrary and dw may be
// odd). A lane keeps an exact 64-bit sum of millimetres and a 32-bit pixel count; the 64 lanes are
// reduced with shuffles, the four waves through LDS, and thread 0 does the double-precision
// epilogue and writes the detection's 8 floats. No atomics, no workspace, no host synchronisation;
// every output row is written by every launch.
#include "common.h"
#include "resample_dev.h"

#include <cmath>

namespace tv {
namespace localize {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCorner = 1 << 30;  // corners are clamped to +-2^30 before the integer conversion

struct Params {
  // box mode
  const float* records;  // [B][K][rec_stride]: y, x, h, w in columns 2-5
  int rec_stride;
  double box_scale;
  // mask mode
  const float* masks;    // [B][K][mh][mw]
  int mh, mw;
  const long long* det;  // [B][K] box row per detection
  const float* box;      // [B][A][4] y, x, h, w
  int A;
  int bound_by_box;
  // both
  const int* counts;     // [B]
  int B, K;
  const uint16_t* depth; // [depth_batch][dh][dw] millimetres
  int depth_batch, dh, dw;
  double fx, fy, cx, cy, min_depth_sum, min_z;
  float* out;            // [B][K][8]
};

struct Region {
  int x0, x1, y0, y1;  // inclusive, clipped to the image; empty when x0 > x1 or y0 > y1
  double ex, ey;
};

// int(v) of the node (truncation toward zero) for a finite or infinite v, with the value clamped
// first so the conversion is always in range. NaN is the caller's case.
__device__ inline int trunc_clamped(double v) {
  v = v < -(double)kCorner ? -(double)kCorner : v;
  v = v > (double)kCorner ? (double)kCorner : v;
  return (int)v;
}

// centernet_node.py:144-157 in double, as the node's Python floats. Contraction is off: a fused
// e_x - s * W rounds once instead of twice and moves the truncated corner (x = 3/64, w = 5/64 at
// dw = 64: 1.0 uncontracted, 0.9999999999999999 fused).
__device__ inline Region box_region(const Params& p, const float* r) {
#pragma clang fp contract(off)
  Region g;
  const double x = (double)r[3], y = (double)r[2], w = (double)r[5], h = (double)r[4];
  g.ex = x * (double)p.dw;
  g.ey = y * (double)p.dh;
  const double W = w * (double)p.dw, H = h * (double)p.dh;
  const double sw = p.box_scale * W, sh = p.box_scale * H;
  const double ax = g.ex - sw, bx = g.ex + sw, ay = g.ey - sh, by = g.ey + sh;
  g.x0 = g.y0 = 0;
  g.x1 = g.y1 = -1;
  // a NaN corner (non-finite x, y, w or h, or inf - inf) selects nothing
  if (!(ax == ax) || !(bx == bx) || !(ay == ay) || !(by == by) || !isfinite(x) || !isfinite(y) || !isfinite(w) ||
      !isfinite(h))
    return g;
  const int cax = trunc_clamped(ax), cbx = trunc_clamped(bx), cay = trunc_clamped(ay), cby = trunc_clamped(by);
  g.x0 = max(min(cax, cbx), 0);
  g.x1 = min(max(cax, cbx), p.dw - 1);
  g.y0 = max(min(cay, cby), 0);
  g.y1 = min(max(cay, cby), p.dh - 1);
  return g;
}

__device__ inline Region mask_region(const Params& p, const float* q) {
#pragma clang fp contract(off)
  Region g;
  g.ex = (double)q[1] * (double)p.dw;  // yolact_node.py:181-182
  g.ey = (double)q[0] * (double)p.dh;
  g.x0 = g.y0 = 0;
  g.x1 = p.dw - 1;
  g.y1 = p.dh - 1;
  if (p.bound_by_box) {
    // the rows and columns that can map into the box crop (resample_dev.h)
    resample::box_crop(q, p.mh, p.mw, p.dh, p.dw, 0.f, g.x0, g.x1, g.y0, g.y1);
  }
  return g;
}

using resample::nearest_src;  // torch's CPU nearest F.interpolate map (resample_dev.h)

template <bool MASK>
__device__ inline void take(unsigned v, int xx, const float* mrow, float scale_w, int mw, unsigned& s, unsigned& c) {
  bool sel = v != 0;
  // the mask value is loaded whether or not the depth is 0 (its address is always inside the mask):
  // a load that waited for the depth value would put two memory round trips in series
  if (MASK) sel = sel & (mrow[nearest_src(xx, scale_w, mw)] > 0.5f);
  s += sel ? v : 0u;
  c += sel ? 1u : 0u;
}

template <bool MASK>
__global__ __launch_bounds__(kThreads) void localize(const Params p) {
  __shared__ unsigned long long ssum[kWaves];
  __shared__ unsigned scnt[kWaves];
  const int b = blockIdx.x / p.K, k = blockIdx.x - b * p.K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = min(max(p.counts[b], 0), p.K);
  bool active = k < n;
  Region g;
  g.x0 = g.y0 = 0;
  g.x1 = g.y1 = -1;
  g.ex = g.ey = 0.0;
  if (active) {
    if (MASK) {
      const long long d = p.det[(size_t)b * p.K + k];
      if (d >= 0 && d < p.A) g = mask_region(p, p.box + ((size_t)b * p.A + (size_t)d) * 4);
      else active = false;  // not a row of `box`: nothing is read
    } else {
      g = box_region(p, p.records + ((size_t)b * p.K + k) * p.rec_stride);
    }
  }
  unsigned long long sum = 0;
  unsigned cnt = 0;
  if (g.x0 <= g.x1 && g.y0 <= g.y1) {
    const uint16_t* img = p.depth + (size_t)(p.depth_batch == 1 ? 0 : b) * p.dh * p.dw;
    const float* mimg = MASK ? p.masks + ((size_t)b * p.K + k) * p.mh * p.mw : nullptr;
    const float scale_w = MASK ? (float)p.mw / (float)p.dw : 0.f;
    const float scale_h = MASK ? (float)p.mh / (float)p.dh : 0.f;
    const int len = g.x1 - g.x0 + 1;
    for (int yy = g.y0 + wave; yy <= g.y1; yy += kWaves) {
      const uint16_t* row = img + (size_t)yy * p.dw + g.x0;
      const float* mrow = MASK ? mimg + (size_t)nearest_src(yy, scale_h, p.mh) * p.mw : nullptr;
      // pixels before the first 16-byte boundary, 8-pixel vectors, then the rest: all inside [0, len)
      const int head = min((int)((8 - ((reinterpret_cast<uintptr_t>(row) >> 1) & 7)) & 7), len);
      const int nvec = (len - head) >> 3;
      const int tail0 = head + 8 * nvec;
      unsigned s = 0, c = 0;  // at most 8 pixels of < 2^16 each before they join the 64-bit sum
      if (lane < head) take<MASK>(row[lane], g.x0 + lane, mrow, scale_w, p.mw, s, c);
      if (lane < len - tail0) take<MASK>(row[tail0 + lane], g.x0 + tail0 + lane, mrow, scale_w, p.mw, s, c);
      sum += s;
      cnt += c;
      for (int v = lane; v < nvec; v += 64) {
        const int e = head + 8 * v;
        const uint4 q = *reinterpret_cast<const uint4*>(row + e);
        const unsigned w4[4] = {q.x, q.y, q.z, q.w};
        s = 0;
        c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          take<MASK>(w4[j] & 0xFFFFu, g.x0 + e + 2 * j, mrow, scale_w, p.mw, s, c);
          take<MASK>(w4[j] >> 16, g.x0 + e + 2 * j + 1, mrow, scale_w, p.mw, s, c);
        }
        sum += s;
        cnt += c;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  if (lane == 0) {
    ssum[wave] = sum;
    scnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < kWaves; ++w) {
    sum += ssum[w];
    cnt += scnt[w];
  }
  {
#pragma clang fp contract(off)
    const double depth_sum = (double)sum / 1000.0;
    const double z = cnt ? (double)sum / (double)cnt / 1000.0 : 0.0;
    const bool valid = active && cnt != 0 && !(depth_sum < p.min_depth_sum) && !(z < p.min_z);
    float x3 = 0.f, y3 = 0.f, z3 = 0.f;
    if (valid) {
      x3 = (float)((g.ex - p.cx) * (z / p.fx));
      y3 = (float)((g.ey - p.cy) * (z / p.fy));
      z3 = (float)z;
    }
    float4* o = reinterpret_cast<float4*>(p.out + (size_t)blockIdx.x * 8);
    o[0] = make_float4(x3, y3, z3, valid ? 1.f : 0.f);
    o[1] = make_float4((float)cnt, (float)depth_sum, (float)g.ex, (float)g.ey);
  }
}

}  // namespace localize

static int launch(bool mask, const localize::Params& p, hipStream_t s) {
  const dim3 grid((unsigned)((long long)p.B * p.K)), block(localize::kThreads);
  if (mask) hipLaunchKernelGGL(localize::localize<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(localize::localize<false>, grid, block, 0, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

static int check_common(const char* what, const void* counts, int B, int K, const void* depth, int depth_batch, int dh,
                        int dw, double fx, double fy, const float* out) {
  const std::string w(what);
  if (!counts || !depth || !out) { set_error(w + ": null pointer"); return 1; }
  if (dh < 1 || dw < 1) { set_error(w + ": depth size must be positive"); return 1; }
  if (depth_batch != 1 && depth_batch != B) { set_error(w + ": depth_batch must be 1 or B"); return 1; }
  if (fx == 0.0 || fy == 0.0) { set_error(w + ": fx and fy must not be 0"); return 1; }
  if ((long long)B * K > 0x7FFFFFFFLL) { set_error(w + ": B * K exceeds the grid limit"); return 1; }
  if (reinterpret_cast<uintptr_t>(depth) & 1) { set_error(w + ": depth must be 2-byte aligned"); return 1; }
  if (reinterpret_cast<uintptr_t>(out) & 15) { set_error(w + ": out must be 16-byte aligned"); return 1; }
  return 0;
}

int launch_localize_boxes(const float* records, int rec_stride, const int* counts, int B, int K, const uint16_t* depth,
                          int depth_batch, int dh, int dw, double box_scale, double fx, double fy, double cx, double cy,
                          double min_depth_sum, double min_z, float* out, hipStream_t s) {
  if (B < 0 || K < 0) { set_error("localize_boxes: negative B or K"); return 1; }
  if ((long long)B * K == 0) return 0;
  if (!records) { set_error("localize_boxes: null pointer"); return 1; }
  if (rec_stride < 6) { set_error("localize_boxes: records need at least 6 columns (y, x, h, w in 2-5)"); return 1; }
  if (int rc = check_common("localize_boxes", counts, B, K, depth, depth_batch, dh, dw, fx, fy, out)) return rc;
  localize::Params p{};
  p.records = records; p.rec_stride = rec_stride; p.box_scale = box_scale;
  p.counts = counts; p.B = B; p.K = K;
  p.depth = depth; p.depth_batch = depth_batch; p.dh = dh; p.dw = dw;
  p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.min_depth_sum = min_depth_sum; p.min_z = min_z;
  p.out = out;
  return launch(false, p, s);
}

int launch_localize_masks(const float* masks, int mh, int mw, const int* counts, const long long* det, const float* box,
                          int A, int B, int n, const uint16_t* depth, int depth_batch, int dh, int dw, int bound_by_box,
                          double fx, double fy, double cx, double cy, double min_depth_sum, double min_z, float* out,
                          hipStream_t s) {
  if (B < 0 || n < 0) { set_error("localize_masks: negative B or n"); return 1; }
  if ((long long)B * n == 0) return 0;
  if (!masks || !det || !box) { set_error("localize_masks: null pointer"); return 1; }
  if (mh < 1 || mw < 1 || A < 1) { set_error("localize_masks: mask size and A must be positive"); return 1; }
  if (int rc = check_common("localize_masks", counts, B, n, depth, depth_batch, dh, dw, fx, fy, out)) return rc;
  localize::Params p{};
  p.masks = masks; p.mh = mh; p.mw = mw; p.det = det; p.box = box; p.A = A; p.bound_by_box = bound_by_box ? 1 : 0;
  p.counts = counts; p.B = B; p.K = n;
  p.depth = depth; p.depth_batch = depth_batch; p.dh = dh; p.dw = dw;
  p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.min_depth_sum = min_depth_sum; p.min_z = min_z;
  p.out = out;
  return launch(true, p, s);
}

}  // namespace tv
