// Training augmentation of u8 camera frames in two launches (the contract is tv_augment_frames' in
// include/tauv_vision_amd.h; the definition, step by step, is DESIGN §20):
//   augment_gray_mean  the contrast step's mean gray of each source frame, as fixed-order partial sums
//   augment_frames     homography warp (one bilinear resampling), colour, noise, box blur, Normalize
// Both are pure functions of (frames, seg, records, seed): no atomics, every sum in a fixed order.
#include "common.h"
#include "resample_dev.h"

// every expression below is evaluated as written: the definition fixes the order of the fp32 operations
// (fused multiply-adds appear only where lin_blend asks for them)
#pragma clang fp contract(off)

namespace tv {
namespace {

constexpr int kRec = 32;  // fp32 slots per record: minv[9], perm[3], brightness, contrast, saturation, hue,
                          // sat_shift, val_shift, noise_sigma, blur_k, zeros
constexpr int kTile = 32;                      // destination tile edge
constexpr int kMaxHalo = 3;                    // blur_k <= 7
constexpr int kRegion = kTile + 2 * kMaxHalo;  // 38
constexpr int kThreads = 256;
// augment_gray_mean: a workgroup sums 4096 pixels, a thread 4 quads of 4 pixels (12 bytes each)
constexpr int kQuadsPerThread = 4;
constexpr int kMeanPixels = kThreads * kQuadsPerThread * 4;

struct AugParams {
  const uint8_t* frames;  // [B, Hs, Ws, 3]
  const uint8_t* seg;     // [B, Hs, Ws] or null
  const float* rec;       // [B, 32]
  double* partial;        // [B, G]
  float* img;             // [B, 3, Hd, Wd]
  uint8_t* seg_out;       // [B, Hd, Wd] or null
  int B, Hs, Ws, Hd, Wd, G;
  uint32_t key0, key1;
  float mean[3], std[3];
};

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ int perm_of(float v) { return min(max((int)v, 0), 2); }
__device__ __forceinline__ float pick(int i, float a, float b, float c) { return i == 0 ? a : i == 1 ? b : c; }

__device__ __forceinline__ float gray_of(float r, float g, float b) {
  return (0.299f * r + 0.587f * g) + 0.114f * b;
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t o[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__device__ __forceinline__ float uniform24(uint32_t o) {
  return ((float)(o >> 8) + 0.5f) * 0x1p-24f;
}

// ---- augment_gray_mean ---------------------------------------------------------------------------
// partial[b, g] = sum over pixels [g * 4096, (g + 1) * 4096) of frame b of gray(clamp(brightness *
// perm(src))), the gray in fp32 and the sum in double: per thread over its quads in order, over the wave
// by xor shuffles, over the four waves in order. Wave 0 of every augment_frames workgroup adds the G partials.
__global__ __launch_bounds__(kThreads) void augment_gray_mean(AugParams P) {
  const int b = blockIdx.y, g = blockIdx.x;
  const float* rec = P.rec + (size_t)b * kRec;
  if (rec[13] == 1.f) return;  // contrast 1: the mean is never read
  const float br = rec[12];
  const int p0 = perm_of(rec[9]), p1 = perm_of(rec[10]), p2 = perm_of(rec[11]);
  const int n = P.Hs * P.Ws;
  const uint8_t* fr = P.frames + (size_t)b * n * 3;
  const bool aligned = ((uintptr_t)fr & 3) == 0;
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int q = (g * kQuadsPerThread + k) * kThreads + (int)threadIdx.x;  // quad: pixels 4q .. 4q + 3
    const int px = q * 4;
    if (px >= n) break;
    uint8_t v[12];
    if (aligned && px + 4 <= n) {
      const uint32_t* w = (const uint32_t*)(fr + (size_t)px * 3);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = (uint8_t)(w0 >> (8 * i));
        v[4 + i] = (uint8_t)(w1 >> (8 * i));
        v[8 + i] = (uint8_t)(w2 >> (8 * i));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = px * 3 + i < n * 3 ? fr[(size_t)px * 3 + i] : (uint8_t)0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (px + i >= n) break;
      const float s0 = (float)v[3 * i], s1 = (float)v[3 * i + 1], s2 = (float)v[3 * i + 2];
      const float r = clamp255(pick(p0, s0, s1, s2) * br), gg = clamp255(pick(p1, s0, s1, s2) * br),
                  bb = clamp255(pick(p2, s0, s1, s2) * br);
      sum += (double)gray_of(r, gg, bb);
    }
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  __shared__ double wave_sum[kThreads / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) P.partial[(size_t)b * P.G + g] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// ---- augment_frames ------------------------------------------------------------------------------
struct FrameRec {
  float m[9];
  int p0, p1, p2;
  float brightness, contrast, saturation, hue, sat_shift, val_shift, sigma, mu;
  int k;
  bool hsv;
};

// steps 1-5 of the definition at destination pixel (y, x) of frame b: the value before the blur (0
// outside the source frame: the padding takes no colour and no noise), `inside`, and the seg value
__device__ __forceinline__ void eval_pixel(const AugParams& P, const FrameRec& F, const uint8_t* fr, const uint8_t* sg,
                                           int b, int y, int x, float c[3], bool& inside, uint8_t& segv) {
  const float X = (float)x + 0.5f, Y = (float)y + 0.5f;
  const float w = (F.m[6] * X + F.m[7] * Y) + F.m[8];
  const float u = ((F.m[0] * X + F.m[1] * Y) + F.m[2]) / w;
  const float v = ((F.m[3] * X + F.m[4] * Y) + F.m[5]) / w;
  inside = w > 0.f && u >= 0.f && u < (float)P.Ws && v >= 0.f && v < (float)P.Hs;
  segv = 254;
  c[0] = c[1] = c[2] = 0.f;
  if (!inside) return;
  if (sg) segv = sg[(size_t)(int)v * P.Ws + (int)u];
  int x0, x1, y0, y1;
  float wx0, wx1, wy0, wy1;
  resample::lin_taps(u - 0.5f, P.Ws, x0, x1, wx0, wx1);
  resample::lin_taps(v - 0.5f, P.Hs, y0, y1, wy0, wy1);
  const uint8_t* r0 = fr + (size_t)y0 * P.Ws * 3;
  const uint8_t* r1 = fr + (size_t)y1 * P.Ws * 3;
  float t[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    t[ch] = resample::lin_blend((float)r0[x0 * 3 + ch], (float)r0[x1 * 3 + ch], (float)r1[x0 * 3 + ch],
                                (float)r1[x1 * 3 + ch], wy0, wy1, wx0, wx1);
  float r = pick(F.p0, t[0], t[1], t[2]), g = pick(F.p1, t[0], t[1], t[2]), bl = pick(F.p2, t[0], t[1], t[2]);
  // brightness, contrast, saturation
  r = clamp255(r * F.brightness);
  g = clamp255(g * F.brightness);
  bl = clamp255(bl * F.brightness);
  if (F.contrast != 1.f) {
    const float o = (1.f - F.contrast) * F.mu;
    r = clamp255(F.contrast * r + o);
    g = clamp255(F.contrast * g + o);
    bl = clamp255(F.contrast * bl + o);
  }
  if (F.saturation != 1.f) {
    const float o = (1.f - F.saturation) * gray_of(r, g, bl);
    r = clamp255(F.saturation * r + o);
    g = clamp255(F.saturation * g + o);
    bl = clamp255(F.saturation * bl + o);
  }
  if (F.hsv) {
    const float rn = r / 255.f, gn = g / 255.f, bn = bl / 255.f;
    const float mx = fmaxf(rn, fmaxf(gn, bn)), mn = fminf(rn, fminf(gn, bn)), d = mx - mn;
    float h = 0.f;
    if (d > 0.f) {
      if (mx == rn) h = (gn - bn) / d;
      else if (mx == gn) h = (bn - rn) / d + 2.f;
      else h = (rn - gn) / d + 4.f;
      h = h / 6.f;
    }
    float s = mx > 0.f ? d / mx : 0.f;
    h = h + F.hue;
    h = h - floorf(h);
    s = clamp01(s + F.sat_shift);
    const float val = clamp01(mx + F.val_shift);
    const float h6 = h * 6.f, vs = val * s;
    float out[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float kk = (float)(5 - 2 * i) + h6;  // n = 5, 3, 1 for R, G, B
      kk = kk >= 6.f ? kk - 6.f : kk;
      kk = kk >= 6.f ? kk - 6.f : kk;
      const float f = fmaxf(0.f, fminf(fminf(kk, 4.f - kk), 1.f));
      out[i] = (val - vs * f) * 255.f;
    }
    r = out[0]; g = out[1]; bl = out[2];
  }
  if (F.sigma != 0.f) {
    uint32_t o[4];
    philox4x32_10((uint32_t)x, (uint32_t)y, (uint32_t)b, 0u, P.key0, P.key1, o);
    const float u0 = uniform24(o[0]), u1 = uniform24(o[1]), u2 = uniform24(o[2]), u3 = uniform24(o[3]);
    const float ra = sqrtf(-2.f * logf(u0)), aa = 6.2831855f * u1;
    const float rb = sqrtf(-2.f * logf(u2)), ab = 6.2831855f * u3;
    r = clamp255(r + F.sigma * (ra * cosf(aa)));
    g = clamp255(g + F.sigma * (ra * sinf(aa)));
    bl = clamp255(bl + F.sigma * (rb * cosf(ab)));
  }
  c[0] = r; c[1] = g; c[2] = bl;
}

// reflect-101 of a position up to (n - 1) outside [0, n); further out it is clamped, which only
// positions that no stored pixel reads can be (the tile's overhang past the frame)
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// One workgroup per 32 x 32 destination tile of one frame. blur_k == 1: every thread evaluates and
// stores its pixels. Otherwise the tile plus a halo of (blur_k - 1) / 2 is evaluated into three LDS
// planes (row pitch = region width: consecutive lanes on consecutive banks), summed along x into a
// second buffer, then along y; each sum in tap order.
__global__ __launch_bounds__(kThreads) void augment_frames(AugParams P) {
  __shared__ float s_p[3][kRegion * kRegion];
  __shared__ float s_h[3][kRegion * kTile];
  __shared__ uint8_t s_in[kTile * kTile];
  const int b = blockIdx.z, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int tid = threadIdx.x;
  const float* rec = P.rec + (size_t)b * kRec;
  FrameRec F;
#pragma unroll
  for (int i = 0; i < 9; ++i) F.m[i] = rec[i];
  F.p0 = perm_of(rec[9]); F.p1 = perm_of(rec[10]); F.p2 = perm_of(rec[11]);
  F.brightness = rec[12]; F.contrast = rec[13]; F.saturation = rec[14];
  F.hue = rec[15]; F.sat_shift = rec[16]; F.val_shift = rec[17];
  F.sigma = rec[18];
  F.k = min(max((int)rec[19], 1), 2 * kMaxHalo + 1) | 1;
  F.hsv = F.hue != 0.f || F.sat_shift != 0.f || F.val_shift != 0.f;
  F.mu = 0.f;
  if (F.contrast != 1.f) {  // (uniform over the workgroup) the last pass of the mean: wave 0 adds the frame's partials,
    __shared__ float s_mu;  // lane l those at l, l + 64, ... in order, then xor shuffles: a fixed order
    if (tid < 64) {
      double sum = 0.0;
      for (int g = tid; g < P.G; g += 64) sum += P.partial[(size_t)b * P.G + g];
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
      if (tid == 0) s_mu = (float)(sum / (double)((long long)P.Hs * P.Ws));
    }
    __syncthreads();
    F.mu = s_mu;
  }
  const uint8_t* fr = P.frames + (size_t)b * P.Hs * P.Ws * 3;
  const uint8_t* sg = P.seg ? P.seg + (size_t)b * P.Hs * P.Ws : nullptr;
  const size_t plane = (size_t)P.Hd * P.Wd;
  float* img = P.img + (size_t)b * 3 * plane;
  uint8_t* so = P.seg_out ? P.seg_out + (size_t)b * plane : nullptr;
  const int lx = tid & (kTile - 1), ly0 = tid / kTile;  // 8 rows of 32 per pass
  const int x = tx0 + lx;

  if (F.k == 1) {
    if (x >= P.Wd) return;
    for (int ly = ly0; ly < kTile; ly += kThreads / kTile) {
      const int y = ty0 + ly;
      if (y >= P.Hd) break;
      float c[3];
      bool inside;
      uint8_t segv;
      eval_pixel(P, F, fr, sg, b, y, x, c, inside, segv);
      const size_t o = (size_t)y * P.Wd + x;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) img[ch * plane + o] = (c[ch] / 255.f - P.mean[ch]) / P.std[ch];
      if (so) so[o] = segv;
    }
    return;
  }

  const int halo = F.k >> 1, rw = kTile + 2 * halo;
  for (int i = tid; i < rw * rw; i += kThreads) {
    const int ry = i / rw, rx = i - ry * rw;
    const int yy = ty0 - halo + ry, xx = tx0 - halo + rx;
    const int y = reflect101(yy, P.Hd), xr = reflect101(xx, P.Wd);
    float c[3];
    bool inside;
    uint8_t segv;
    eval_pixel(P, F, fr, sg, b, y, xr, c, inside, segv);
    s_p[0][i] = c[0];
    s_p[1][i] = c[1];
    s_p[2][i] = c[2];
    const int cy = ry - halo, cx = rx - halo;
    if (cy >= 0 && cy < kTile && cx >= 0 && cx < kTile) {
      s_in[cy * kTile + cx] = inside ? 1 : 0;
      if (so && yy < P.Hd && xx < P.Wd) so[(size_t)yy * P.Wd + xx] = segv;
    }
  }
  __syncthreads();
  // along x: s_h[ch][ry][lx] = sum over taps of s_p[ch][ry][lx .. lx + k - 1]
  for (int i = tid; i < rw * kTile; i += kThreads) {
    const int ry = i / kTile, cx = i - ry * kTile;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* row = &s_p[ch][ry * rw + cx];
      float acc = row[0];
      for (int t = 1; t < F.k; ++t) acc += row[t];
      s_h[ch][i] = acc;
    }
  }
  __syncthreads();
  if (x >= P.Wd) return;
  const float area = (float)(F.k * F.k);
  for (int ly = ly0; ly < kTile; ly += kThreads / kTile) {
    const int y = ty0 + ly;
    if (y >= P.Hd) break;
    const bool inside = s_in[ly * kTile + lx] != 0;
    const size_t o = (size_t)y * P.Wd + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* col = &s_h[ch][ly * kTile + lx];
      float acc = col[0];
      for (int t = 1; t < F.k; ++t) acc += col[t * kTile];
      const float q = inside ? acc / area : 0.f;
      img[ch * plane + o] = (q / 255.f - P.mean[ch]) / P.std[ch];
    }
  }
}

int mean_groups(long long pixels) { return (int)((pixels + kMeanPixels - 1) / kMeanPixels); }

}  // namespace

int augment_workspace_size(int B, int src_h, int src_w, long long* bytes) {
  if (!bytes || B < 1 || src_h < 1 || src_w < 1 || (long long)src_h * src_w * 3 >= (1LL << 31)) {
    set_error("augment: bad shapes");
    return 1;
  }
  const long long b = (long long)B * mean_groups((long long)src_h * src_w) * (long long)sizeof(double);
  *bytes = (b + 15) / 16 * 16;
  return 0;
}

int launch_augment_frames(const uint8_t* frames, const uint8_t* seg, int B, int Hs, int Ws, int Hd, int Wd,
                          const float* records, unsigned long long seed, const float* mean, const float* std,
                          float* img_out, uint8_t* seg_out, void* ws, long long ws_bytes, hipStream_t s) {
  long long need = 0;
  if (int rc = augment_workspace_size(B, Hs, Ws, &need)) return rc;
  if (!frames || !records || !mean || !std || !img_out || !ws) { set_error("augment: null argument"); return 1; }
  if ((seg == nullptr) != (seg_out == nullptr)) { set_error("augment: seg and seg_out go together"); return 1; }
  if (Hd < 1 || Wd < 1 || (long long)Hd * Wd >= (1LL << 31) || B > 65535) { set_error("augment: bad shapes"); return 1; }
  if (ws_bytes < need || ((uintptr_t)ws & 7)) { set_error("augment: workspace too small or misaligned"); return 1; }
  for (int c = 0; c < 3; ++c)
    if (!(std[c] != 0.f)) { set_error("augment: std must be non-zero"); return 1; }
  AugParams P{};
  P.frames = frames; P.seg = seg; P.rec = records; P.partial = (double*)ws; P.img = img_out; P.seg_out = seg_out;
  P.B = B; P.Hs = Hs; P.Ws = Ws; P.Hd = Hd; P.Wd = Wd; P.G = mean_groups((long long)Hs * Ws);
  P.key0 = (uint32_t)seed; P.key1 = (uint32_t)(seed >> 32);
  for (int c = 0; c < 3; ++c) { P.mean[c] = mean[c]; P.std[c] = std[c]; }
  const unsigned gy = (unsigned)((Hd + kTile - 1) / kTile);
  if (gy > 65535) { set_error("augment: bad shapes"); return 1; }
  hipLaunchKernelGGL(augment_gray_mean, dim3((unsigned)P.G, (unsigned)B), dim3(kThreads), 0, s, P);
  TV_HIP(hipGetLastError());
  hipLaunchKernelGGL(augment_frames, dim3((unsigned)((Wd + kTile - 1) / kTile), gy, (unsigned)B), dim3(kThreads), 0, s,
                     P);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
