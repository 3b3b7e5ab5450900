// The bandwidth kernels of the ResNet-18 backbone (gfx950; planner_resnet.cpp). All NHWC, one lane
// per 16-byte channel vector, consecutive lanes on consecutive vectors, so a wave's loads and stores
// are whole runs of contiguous 16-byte vectors; arithmetic in fp32, one rounding to the compute dtype.
//   maxpool3x3s2  MaxPool2d(3, 2, 1), floor mode (torchvision resnet.py `maxpool`): taps outside the
//                 image are ignored (-inf padding, not zero)
//   add_relu      relu(a + b): the residual add of a block whose bn2 output is tapped
//   store_f32     a compute-dtype tensor into the caller's fp32 buffer, exactly (the taps of
//                 TV_ARCH_RESNET18, which stay in the arena for the next layer's add)
//   stem7s2_pool  conv1 + bn1 + ReLU + the max-pool from the fp32 NCHW image, or from u8 NHWC camera frames
//                 (ToTensor + Normalize through a LUT), in one launch (fp16 / bf16)
#include <algorithm>

#include "conv_common.h"

namespace tv {
namespace rn {

template <typename T>
struct Vec16 {
  static constexpr int N = 16 / (int)sizeof(T);
  union {
    uint4 u;
    T e[N];
  };
};

// lane -> (frame, output pixel, channel vector); grid and vectorisation as dla::maxpool2_ceil
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2(const T* __restrict__ src, int B, int H, int W, int C,
                                                    T* __restrict__ out, int Ho, int Wo) {
  constexpr int V = Vec16<T>::N;
  const int nq = C / V;
  const unsigned total = (unsigned)B * Ho * Wo * nq;  // < 2^31 (checked by the launcher)
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  // 32-bit index math: 64-bit division is a long software sequence on CDNA
  const unsigned q = i % (unsigned)nq;
  const unsigned pix = i / (unsigned)nq;
  const unsigned ox = pix % (unsigned)Wo;
  const unsigned r = pix / (unsigned)Wo;
  const unsigned oy = r % (unsigned)Ho;
  const unsigned b = r / (unsigned)Ho;
  float m[V];
#pragma unroll
  for (int e = 0; e < V; ++e) m[e] = -__builtin_inff();
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int y = 2 * (int)oy - 1 + dy, x = 2 * (int)ox - 1 + dx;
      if (y >= 0 && y < H && x >= 0 && x < W) {  // (the centre tap is always inside: Ho = (H - 1) / 2 + 1)
        Vec16<T> t;
        t.u = *reinterpret_cast<const uint4*>(src + (((size_t)b * H + y) * W + x) * C + q * V);
#pragma unroll
        for (int e = 0; e < V; ++e) m[e] = fmaxf(m[e], (float)t.e[e]);
      }
    }
  Vec16<T> o;
#pragma unroll
  for (int e = 0; e < V; ++e) o.e[e] = (T)m[e];
  *reinterpret_cast<uint4*>(out + (size_t)pix * C + q * V) = o.u;
}

template <typename T>
__global__ __launch_bounds__(256) void add_relu(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                size_t nvec) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvec) return;
  Vec16<T> x, y, o;
  x.u = reinterpret_cast<const uint4*>(a)[i];
  y.u = reinterpret_cast<const uint4*>(b)[i];
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) o.e[e] = (T)fmaxf((float)x.e[e] + (float)y.e[e], 0.f);
  reinterpret_cast<uint4*>(out)[i] = o.u;
}

// one lane per 16-byte vector of the source: 16 (fp32) or 32 (fp16 / bf16) bytes of output
template <typename T>
__global__ __launch_bounds__(256) void store_f32(const T* __restrict__ src, float* __restrict__ out, size_t nvec) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvec) return;
  constexpr int V = Vec16<T>::N;
  Vec16<T> x;
  x.u = reinterpret_cast<const uint4*>(src)[i];
  float4* o = reinterpret_cast<float4*>(out + i * V);
#pragma unroll
  for (int k = 0; k < V / 4; ++k)
    o[k] = make_float4((float)x.e[4 * k], (float)x.e[4 * k + 1], (float)x.e[4 * k + 2], (float)x.e[4 * k + 3]);
}

// ---- stem7s2_pool: conv1 7x7 / s2 / p3 (3 -> 64) + bn1 + ReLU + MaxPool2d(3, 2, 1) in one launch ----
// Reads the fp32 NCHW image (IN = 0) or u8 NHWC frames (IN = 1: ToTensor + ImageNet Normalize through a
// 768-entry LUT in LDS, yolact_node.py:109-111 at the model size) and writes only the pooled 64-channel
// tensor: neither the row-expanded staging tensor nor the conv output reaches HBM. A workgroup (4 waves)
// walks tiles of kTH x kTW pooled pixels on a persistent grid, the folded weights resident in LDS:
//   1. the tile's input window (kIR x kIC pixels, zero outside the image) -> LDS as T, pixel-major
//      [row][x * 3 + c]: the 21 values of one kernel row of a conv position are contiguous there;
//   2. the (2 kTH + 1) x (2 kTW + 1) = 117 conv positions the tile's windows cover as a GEMM on
//      mfma_32x32x16: A = weights [64 channels][K], B = patches [K][128 positions, 32 per wave],
//      K = 7 kernel rows x 24 (21 + 3 zero weights, the engine's row-expanded packing) -> 11 k-steps;
//      accumulator columns are positions (one per lane), rows channels;
//   3. + shift, ReLU, one rounding to T -> the conv tile in LDS. A position outside the conv image
//      (the pool's padding: row / column -1, and row CH of an odd CH) stores 0: every window holds
//      its centre, which is inside, and every value inside is >= 0 after the ReLU, so a 0 never
//      changes the max — the same result as leaving the position out;
//   4. 3x3 / s2 max over the conv tile -> the pooled tensor, one 16-byte channel vector per lane.
constexpr int kTH = 4, kTW = 6;                        // pooled tile
constexpr int kCR = 2 * kTH + 1, kCC = 2 * kTW + 1;    // conv positions of a tile: 9 x 13 = 117 (<= 128)
constexpr int kIR = 2 * kCR + 5, kIC = 2 * kCC + 5;    // input window: 23 x 31 pixels
constexpr int kIRS = 96;   // halves per staged input row: 3 kIC = 93, and the last conv column's 24-wide read ends at 6 (kCC - 1) + 24
constexpr int kIRows = kIR + 1;                        // + one zero row: k-step 10's upper half is kernel row 7 (zero weights)
constexpr int kKS = 11, kWS = 184;                     // k-steps of 16; halves per weight row in LDS (176 + 8: 16-byte rows, spread banks)
constexpr int kCS = 72;                                // halves per conv-tile row in LDS (64 + 8)
constexpr int kStemLds = (64 * kWS + kIRows * kIRS + 128 * kCS) * 2;
constexpr int kStemLdsU8 = kStemLds + 768 * 2;         // + the u8 LUT: 48,128 B, three workgroups per CU still fit
constexpr int kRowDw = 25;  // aligned dwords that cover a staged row's 96 bytes at any byte alignment of its first

__constant__ float kMean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float kStd[3] = {0.229f, 0.224f, 0.225f};

struct StemPoolArgs {
  const void* img;       // IN = 0: fp32 NCHW [B, 3, H, W]; IN = 1: u8 NHWC [B, H, W, 3], any byte alignment
  const void* w;         // T [>= 64][Kpad], K = ky * 24 + kx * 3 + c (zero elsewhere), BatchNorm folded
  const float* bias;     // [64]
  void* out;             // T NHWC [B, PH, PW, 64]
  int B, H, W, CH, CW, PH, PW, Kpad, tiles_y, tiles_x;
};

template <typename T, int IN>
__global__ __launch_bounds__(256) void stem7s2_pool(StemPoolArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  T* wl = reinterpret_cast<T*>(lds);
  T* il = wl + 64 * kWS;
  T* cl = il + kIRows * kIRS;
  T* lut = cl + 128 * kCS;  // (IN = 1 only: kStemLdsU8)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 64 * (kKS * 2); i += 256) {  // 16-byte chunks of the 64 x 176 weights
    const int n = i / (kKS * 2), c = i % (kKS * 2);
    *reinterpret_cast<uint4*>(wl + n * kWS + c * 8) = *reinterpret_cast<const uint4*>((const T*)p.w + (size_t)n * p.Kpad + c * 8);
  }
  if constexpr (IN == 1) {
    for (int i = tid; i < 768; i += 256) {
      const int v = i / 3, c = i - v * 3;
      lut[i] = (T)(((float)v / 255.0f - kMean[c]) / kStd[c]);  // prep_u8's expression, bit for bit
    }
    __syncthreads();  // the staging of the first tile reads the LUT
  }
  // this lane's conv position within a tile (positions past the 117th repeat position 0; never pooled)
  const int pos = wave * 32 + (lane & 31), h = lane >> 5;
  const int pc = pos < kCR * kCC ? pos : 0;
  const int pcy = pc / kCC, pcx = pc % kCC;
  const int tiles = p.B * p.tiles_y * p.tiles_x;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int b = t / (p.tiles_y * p.tiles_x), tr = t % (p.tiles_y * p.tiles_x);
    const int py0 = (tr / p.tiles_x) * kTH, px0 = (tr % p.tiles_x) * kTW;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;  // first conv position (pool padding 1)
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;  // first input pixel (conv padding 3)
#ifdef TV_STEM_U8_BYTES
    // timing-only variant (make BUILD=build_x LIBDIR=lib_x EXTRA=-DTV_STEM_U8_BYTES): the simplest u8 staging,
    // one byte load per staged element as the fp32 instance's one value; measured slower (0.37
    // against 0.27 ms per 32 frames)
    if constexpr (IN == 1) {
      const uint8_t* fr = (const uint8_t*)p.img + (size_t)b * p.H * p.W * 3;
      for (int i = tid; i < kIRows * kIRS; i += 256) {
        const int r = i / kIRS, e = i % kIRS, x = e / 3, c = e % 3;
        const int y = iy0 + r, xx = ix0 + x;
        const bool ok = r < kIR && x < kIC && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
        il[i] = ok ? lut[(int)fr[((size_t)y * p.W + xx) * 3 + c] * 3 + c] : (T)0;
      }
    } else
#endif
    if constexpr (IN == 1) {
      // A window row is the contiguous byte span [(y W + ix0) 3, + 93) of the frame, in the LDS row's own
      // order. It is read as the aligned dwords that cover it, aligned from the span's own address (the
      // base may have any byte alignment), one (row, dword) per lane and step, all loads issued before the
      // first LDS write. Only a dword that holds a byte of the image row is loaded (such a dword lies
      // inside the allocation); every element outside the image, past column kIC or in the zero row
      // stages (T)0, not lut[0]: the padding is zero after normalisation.
      constexpr int NS = (kIRows * kRowDw + 255) / 256;
      const int elo = 3 * max(0, -ix0), ehi = 3 * min(kIC, p.W - ix0);  // the row's elements inside the image
      uint32_t raw[NS];
      int e0[NS];  // the dword's first byte as an element of its row (-3 .. 96)
      bool ld[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int i = tid + 256 * k, r = i / kRowDw, d = i - r * kRowDw, y = iy0 + r;
        const bool rok = i < kIRows * kRowDw && r < kIR && y >= 0 && y < p.H;
        const uint8_t* row = (const uint8_t*)p.img + (((long)b * p.H + (rok ? y : 0)) * p.W + ix0) * 3;
        e0[k] = 4 * d - (int)((uintptr_t)row & 3);
        ld[k] = rok && e0[k] + 4 > elo && e0[k] < ehi;  // some byte of the dword is inside the image
        raw[k] = ld[k] ? *reinterpret_cast<const uint32_t*>(row + e0[k]) : 0u;
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int i = tid + 256 * k, r = i / kRowDw;
        if (i >= kIRows * kRowDw) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = e0[k] + j;
          if (e < 0 || e >= kIRS) continue;
          il[r * kIRS + e] = ld[k] && e >= elo && e < ehi ? lut[(int)((raw[k] >> (8 * j)) & 255u) * 3 + e % 3] : (T)0;
        }
      }
    } else {
      const float* im = (const float*)p.img + (size_t)b * 3 * p.H * p.W;
      for (int i = tid; i < kIRows * kIRS; i += 256) {
        const int r = i / kIRS, e = i % kIRS, x = e / 3, c = e % 3;
        const int y = iy0 + r, xx = ix0 + x;
        float v = 0.f;
        if (r < kIR && x < kIC && y >= 0 && y < p.H && xx >= 0 && xx < p.W) v = im[((size_t)c * p.H + y) * p.W + xx];
        il[i] = (T)v;
      }
    }
    __syncthreads();  // the window (and, the first time, the weights) staged; the previous tile's pooling done
    f32x16 acc[2] = {};
#pragma unroll
    for (int s = 0; s < kKS; ++s) {
      const int k0 = 16 * s + 8 * h, ky = k0 / 24, off = k0 % 24;
      // 8 consecutive K values: halves (2 pcy + ky) kIRS + 6 pcx + off ..., an even offset: 4-byte reads
      const uint32_t* src = reinterpret_cast<const uint32_t*>(il + (2 * pcy + ky) * kIRS + 6 * pcx + off);
      const uint4 bf = make_uint4(src[0], src[1], src[2], src[3]);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const uint4 af = *reinterpret_cast<const uint4*>(wl + (32 * nt + (lane & 31)) * kWS + k0);
        Mfma<T>::run(af, bf, acc[nt]);
      }
    }
    const int cy = cy0 + pcy, cx = cx0 + pcx;
    const bool inside = pos < kCR * kCC && cy >= 0 && cy < p.CH && cx >= 0 && cx < p.CW;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {  // registers 4g .. 4g + 3: channels 32 nt + 8 g + 4 h + (0..3)
        const int n0 = 32 * nt + 8 * g + 4 * h;
        T v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (T)(inside ? fmaxf(acc[nt][4 * g + e] + p.bias[n0 + e], 0.f) : 0.f);
        *reinterpret_cast<uint2*>(cl + pos * kCS + n0) = *reinterpret_cast<const uint2*>(v);
      }
    __syncthreads();  // the conv tile complete
    if (tid < kTH * kTW * 8) {
      const int q = tid & 7, pp = tid >> 3, py = pp / kTW, px = pp % kTW;
      if (py0 + py < p.PH && px0 + px < p.PW) {
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = 0.f;  // (every value is >= 0)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            Vec16<T> t;
            t.u = *reinterpret_cast<const uint4*>(cl + ((2 * py + dy) * kCC + 2 * px + dx) * kCS + q * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)t.e[e]);
          }
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = (T)m[e];
        *reinterpret_cast<uint4*>((T*)p.out + (((size_t)b * p.PH + py0 + py) * p.PW + px0 + px) * 64 + q * 8) = o.u;
      }
    }
  }
}

}  // namespace rn

namespace {

bool aligned16(const void* p) { return p && !((uintptr_t)p & 15); }

template <typename T>
int maxpool_t(const void* src, int B, int H, int W, int C, void* out, int Ho, int Wo, hipStream_t s) {
  const long n = (long)B * Ho * Wo * (C / rn::Vec16<T>::N);
  hipLaunchKernelGGL(rn::maxpool3x3s2<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const T*)src, B, H, W, C,
                     (T*)out, Ho, Wo);
  TV_HIP(hipGetLastError());
  return 0;
}
template <typename T>
int add_relu_t(const void* a, const void* b, void* out, size_t nvec, hipStream_t s) {
  hipLaunchKernelGGL(rn::add_relu<T>, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, (const T*)a, (const T*)b,
                     (T*)out, nvec);
  TV_HIP(hipGetLastError());
  return 0;
}
template <typename T>
int store_f32_t(const void* src, float* out, size_t nvec, hipStream_t s) {
  hipLaunchKernelGGL(rn::store_f32<T>, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, (const T*)src, out, nvec);
  TV_HIP(hipGetLastError());
  return 0;
}

#define TV_RN_DISPATCH(dtype, FN, ...)                      \
  do {                                                      \
    if ((dtype) == F32) return FN<float>(__VA_ARGS__);      \
    if ((dtype) == F16) return FN<_Float16>(__VA_ARGS__);   \
    return FN<__bf16>(__VA_ARGS__);                         \
  } while (0)

}  // namespace

int launch_maxpool3x3s2(const void* src, int B, int H, int W, int C, void* out, int dtype, hipStream_t s) {
  if (dtype < F32 || dtype > BF16 || !aligned16(src) || !aligned16(out) || B < 1 || H < 1 || W < 1 || C < 1 ||
      C % (16 / dtype_size(dtype))) {
    set_error("maxpool3x3s2: channels must be whole 16-byte vectors of 16-byte aligned tensors");
    return 1;
  }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  // one lane per output vector, 32-bit lane indices
  if ((long)B * Ho * Wo * (C / (16 / dtype_size(dtype))) >= (1L << 31)) {
    set_error("maxpool3x3s2: too many elements for one launch");
    return 1;
  }
  TV_RN_DISPATCH(dtype, maxpool_t, src, B, H, W, C, out, Ho, Wo, s);
}

namespace {
// n elements as whole 16-byte vectors of the compute dtype, within one launch's blocks
bool vectors(long long n, int dtype, size_t* nvec) {
  if (dtype < F32 || dtype > BF16) return false;
  const int vec = 16 / dtype_size(dtype);
  if (n < 1 || n % vec) return false;
  *nvec = (size_t)(n / vec);
  return (*nvec + 255) / 256 < (1ull << 31);
}
}  // namespace

int launch_add_relu(const void* a, const void* b, void* out, long long n, int dtype, hipStream_t s) {
  size_t nvec = 0;
  if (!vectors(n, dtype, &nvec) || !aligned16(a) || !aligned16(b) || !aligned16(out)) {
    set_error("add_relu: whole 16-byte vectors of 16-byte aligned tensors");
    return 1;
  }
  TV_RN_DISPATCH(dtype, add_relu_t, a, b, out, nvec, s);
}

int launch_stem7s2_pool(const StemPoolParams& q, int dtype, int cu_count, hipStream_t s) {
  const int CH = (q.H - 1) / 2 + 1, CW = (q.W - 1) / 2 + 1, PH = (CH - 1) / 2 + 1, PW = (CW - 1) / 2 + 1;
  if ((dtype != F16 && dtype != BF16) || !q.img || !aligned16(q.w) || !q.bias || !aligned16(q.out) || q.B < 1 ||
      q.H < 1 || q.W < 1 || q.Kpad < 16 * rn::kKS || q.Kpad % 8 ||
      (size_t)q.B * 3 * q.H * q.W >= (1ull << 31) || (size_t)q.B * PH * PW * 64 >= (1ull << 31)) {
    set_error("stem7s2_pool: fp16 / bf16, 16-byte aligned weights of >= 176 K values per row, < 2^31 elements");
    return 1;
  }
  rn::StemPoolArgs a{q.img, q.w, q.bias, q.out, q.B, q.H, q.W, CH, CW, PH, PW, q.Kpad,
                     (PH + rn::kTH - 1) / rn::kTH, (PW + rn::kTW - 1) / rn::kTW};
  const long tiles = (long)a.B * a.tiles_y * a.tiles_x;
  // three workgroups per CU fit by LDS (43 KiB each); the tiles of one workgroup amortise its weight load
  const unsigned grid = (unsigned)std::min<long>(tiles, 3L * std::max(1, cu_count));
  if (q.u8) {
    if (dtype == F16)
      hipLaunchKernelGGL((rn::stem7s2_pool<_Float16, 1>), dim3(grid), dim3(256), rn::kStemLdsU8, s, a);
    else
      hipLaunchKernelGGL((rn::stem7s2_pool<__bf16, 1>), dim3(grid), dim3(256), rn::kStemLdsU8, s, a);
  } else if (dtype == F16) {
    hipLaunchKernelGGL((rn::stem7s2_pool<_Float16, 0>), dim3(grid), dim3(256), rn::kStemLds, s, a);
  } else {
    hipLaunchKernelGGL((rn::stem7s2_pool<__bf16, 0>), dim3(grid), dim3(256), rn::kStemLds, s, a);
  }
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_store_f32(const void* src, float* out, long long n, int dtype, hipStream_t s) {
  size_t nvec = 0;
  if (!vectors(n, dtype, &nvec) || !aligned16(src) || !aligned16(out)) {
    set_error("store_f32: whole 16-byte vectors of 16-byte aligned tensors");
    return 1;
  }
  TV_RN_DISPATCH(dtype, store_f32_t, src, out, nvec, s);
}

}  // namespace tv
