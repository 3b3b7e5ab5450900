// The two bandwidth kernels of the YOLACT neck and head (gfx950):
//  * bilinear_add: the FeaturePyramid's top-down step (feature_pyramid.py:49-50),
//    pyramid[i] = lateral[i] + F.interpolate(pyramid[i + 1], size of lateral[i], mode="bilinear"),
//    NHWC, in place on the lateral conv's output;
//  * head_scatter: one level's raw fp32 head tensors (the final 3x3 convs' accumulators as the
//    GEMMs' fp32 store wrote them) into the caller's three anchor-indexed outputs
//    (prediction_head.py:111-141 + the torch.cat of model.py:55-57), tanh on the mask coefficients.
#include "common.h"
#include "resample_dev.h"

#include <type_traits>

// expression order as torch's ops (explicit __fmaf_rn where torch's CPU kernel fuses)
#pragma clang fp contract(off)

namespace tv {
namespace yh {

using resample::lin_index;  // torch's upsample_bilinear2d source index and weights (resample_dev.h)

template <typename T>
struct Vec16 {
  static constexpr int N = 16 / (int)sizeof(T);
  union {
    uint4 u;
    T e[N];
  };
};

// One lane per (destination pixel, 16-byte channel vector): consecutive lanes walk the channels of
// a pixel, then the next pixel of the row, so the destination read-modify-write is one contiguous
// stream and each of the four source taps a contiguous run per pixel (rows of four taps; the small
// upper level — a quarter of the destination — is re-read from cache). fp32 blend, then one
// rounding of the interpolated value to T (what F.interpolate returns) and one of the sum.
template <typename T>
__global__ __launch_bounds__(256) void bilinear_add(const T* __restrict__ src, int hs, int ws, int src_ldc,
                                                    T* __restrict__ dst, int hd, int wd, int dst_ldc, int chunks,
                                                    float sh, float sw, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % chunks) * Vec16<T>::N;
  const size_t pix = i / chunks;  // (b * hd + y) * wd + x
  const int x = (int)(pix % wd);
  const size_t by = pix / wd;
  const int y = (int)(by % hd);
  const size_t b = by / hd;
  int h0, h1, w0, w1;
  float a0, a1, b0, b1;
  lin_index(y, hs, sh, h0, h1, a0, a1);
  lin_index(x, ws, sw, w0, w1, b0, b1);
  const T* f = src + b * hs * ws * src_ldc + c;
  Vec16<T> A, Bv, C, D, o;
  A.u = *reinterpret_cast<const uint4*>(f + ((size_t)h0 * ws + w0) * src_ldc);
  Bv.u = *reinterpret_cast<const uint4*>(f + ((size_t)h0 * ws + w1) * src_ldc);
  C.u = *reinterpret_cast<const uint4*>(f + ((size_t)h1 * ws + w0) * src_ldc);
  D.u = *reinterpret_cast<const uint4*>(f + ((size_t)h1 * ws + w1) * src_ldc);
  T* d = dst + pix * dst_ldc + c;
  o.u = *reinterpret_cast<const uint4*>(d);
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float t0 = __fmaf_rn((float)A.e[e], b0, (float)Bv.e[e] * b1);
    const float t1 = __fmaf_rn((float)C.e[e], b0, (float)D.e[e] * b1);
    const T up = (T)__fmaf_rn(t0, a0, t1 * a1);
    o.e[e] = (T)((float)o.e[e] + (float)up);
  }
  *reinterpret_cast<uint4*>(d) = o.u;
}

// One lane per fp32 value of the level's (up to three) parts: lane -> (part, frame, pixel, column).
// The level's whole output is a few hundred KiB at most (550 x 550: 4761 anchors x 20 columns), so
// the 4-byte accesses are not worth a vector path (the column counts are arbitrary: n_ar (C + 1)).
__global__ __launch_bounds__(256) void head_scatter(HeadScatterParams p, int n_all) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.B * p.HW * n_all) return;
  int j = (int)(i % n_all);
  const size_t pix = i / n_all;  // b * HW + px
  const int px = (int)(pix % p.HW);
  const size_t b = pix / p.HW;
  int k = 0;
  while (k + 1 < p.nparts && j >= p.part[k].n) j -= p.part[k++].n;
  const HeadScatterPart& q = p.part[k];
  float v = q.src[pix * q.ldc + q.c0 + j];
  if (q.tanh) v = tanhf(v);
  q.dst[b * q.dst_frame + (size_t)px * q.n + j] = v;
}

}  // namespace yh

int launch_bilinear_add(const void* src, int B, int hs, int ws, int src_ldc, void* dst, int hd, int wd, int dst_ldc,
                        int C, int dtype, hipStream_t s) {
  const int vec = 16 / dtype_size(dtype);
  if (!src || !dst || B < 1 || hs < 1 || ws < 1 || hd < 1 || wd < 1 || C < 1 || dtype < F32 || dtype > BF16 ||
      C % vec || src_ldc % vec || dst_ldc % vec || src_ldc < C || dst_ldc < C || ((uintptr_t)src & 15) ||
      ((uintptr_t)dst & 15)) {
    set_error("bilinear_add: channels and pixel strides must be whole 16-byte vectors (16-byte aligned tensors)");
    return 1;
  }
  const int chunks = C / vec;
  const size_t total = (size_t)B * hd * wd * chunks;
  if ((total + 255) / 256 >= (1ull << 31)) {
    set_error("bilinear_add: too many elements for one launch");
    return 1;
  }
  const float sh = (float)hs / (float)hd, sw = (float)ws / (float)wd;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == F32)
    hipLaunchKernelGGL(yh::bilinear_add<float>, grid, dim3(256), 0, s, (const float*)src, hs, ws, src_ldc, (float*)dst,
                       hd, wd, dst_ldc, chunks, sh, sw, total);
  else if (dtype == F16)
    hipLaunchKernelGGL(yh::bilinear_add<_Float16>, grid, dim3(256), 0, s, (const _Float16*)src, hs, ws, src_ldc,
                       (_Float16*)dst, hd, wd, dst_ldc, chunks, sh, sw, total);
  else
    hipLaunchKernelGGL(yh::bilinear_add<__bf16>, grid, dim3(256), 0, s, (const __bf16*)src, hs, ws, src_ldc,
                       (__bf16*)dst, hd, wd, dst_ldc, chunks, sh, sw, total);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_head_scatter(const HeadScatterParams& p, hipStream_t s) {
  int n_all = 0;
  bool ok = p.nparts >= 1 && p.nparts <= kScatterMaxParts && p.B >= 1 && p.HW >= 1;
  for (int k = 0; ok && k < p.nparts; ++k) {
    const HeadScatterPart& q = p.part[k];
    ok = q.src && q.dst && q.n >= 1 && q.c0 >= 0 && q.c0 + q.n <= q.ldc && q.dst_frame >= (long long)p.HW * q.n;
    n_all += q.n;
  }
  const size_t total = (size_t)p.B * p.HW * n_all;
  if (!ok || (total + 255) / 256 >= (1ull << 31)) {
    set_error("head_scatter: bad parts");
    return 1;
  }
  hipLaunchKernelGGL(yh::head_scatter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, n_all);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
