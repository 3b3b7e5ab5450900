// ConvTranspose2d(k = s, stride = s) + pad_to_match + skip add (gfx950, fp16 / bf16) — the
// IDAUp / IDAUpReverse up-path of the reference: `f_i + pad_to_match(up(project(x)), f_i)`
// (dla.py:265-284, 340-357, pad_to_match :195-209, including its H/W-swapped F.pad quirk,
// folded into the target shift (sy, sx) by the planner).
//
// A k = s transposed conv is a per-pixel linear map: input pixel (iy, ix) produces the s x s
// block of target pixels (iy*s + py + sy, ix*s + px + sx), one 128-channel GEMM row per phase
// (py, px). Per phase it is a GEMM [input pixels] x [128 x 128], K = 128, and the pass is bound
// by HBM: per input pixel and phase it reads 256 B of skip tensor and writes 256 B (the 256 B of
// input pixel come from L2 after the first phase). The generic implicit GEMM staged that
// through a 3-slot LDS ring and an fp32 LDS epilogue per 256-pixel tile (2.7 TB/s). Here:
//  * a 512-thread workgroup owns one phase group and a run of 32-pixel tiles; the group's weights
//    (128 x 128 per phase, 34 KiB with a conflict-free 272 B row pitch) move to LDS once, their
//    rows permuted so that MFMA column n of channel fragment i is output channel 4n + i;
//  * each wave streams its own tiles with no barrier. Pixels are the MFMA rows (the A operand,
//    8 x 16 B of the pixel's channels per lane, straight from global memory) and the phase's
//    weights the columns (the B operand, from LDS): accumulator register r of the four channel
//    fragments then holds, across lanes 0-31, the 128 consecutive channels of pixel 8(r/4) + r%4
//    and across lanes 32-63 those of the pixel four further on, 4 channels = 8 B per lane;
//  * so every skip load and every store of a wave covers the whole 256 B of two target pixels
//    (four whole 128 B lines) instead of 32 B of each of 32 pixels: every line is requested once,
//    not by four instructions a quarter at a time. A lane learns the target pixel of its register
//    from the lane that computed it (two scalar lane reads and a select). Pixels with no target
//    (a partial tile, a cropped row or column) load pixel 0 and store past the range of the
//    output's buffer descriptor, so no access sits behind a branch and the compiler keeps counted
//    vmcnt waits. Skip rows are loaded one step ahead, before the previous step's stores, so
//    waiting for them never waits for those stores (vector memory completes in issue order);
//  * the epilogue works on the accumulators in place (bias, + skip in fp32, one rounding), in the
//    same arithmetic order as conv_pipe's mode-1 epilogue: (acc + bias) + skip. Swapping the MFMA
//    operand roles transposes the product and leaves each element's sum over K as it was.
#include "conv_common.h"

namespace tv {
namespace convt {

constexpr int NT = 512;        // 8 waves
constexpr int NW = NT / 64;
constexpr int C = 128;         // output channels per phase (4 MFMA row tiles)
constexpr int KJ = 8;          // K = 128 input channels = 8 MFMA k-steps of 16
constexpr int WPITCH = 272;    // LDS weight row pitch (bytes): odd multiple of 16 -> no bank conflicts
constexpr int PW = C * WPITCH; // one phase's weights
constexpr int NPG = 4;         // phases per workgroup on large inputs: the input tile is loaded once for all
template <int NP>
constexpr int lds_bytes() { return NP * (PW + C * 4); }
// the last byte a lane reads of a phase's weights (row 3*32 + 31, lane half 1, k-step KJ - 1) is the
// phase's own: no LDS address leaves the launch's allocation (weights, then NP * C bias floats)
static_assert((C - 1) * WPITCH + 16 + (KJ - 1) * 32 + 16 <= PW, "weight reads stay inside the phase");

template <typename T>
__device__ __forceinline__ float lo_f(unsigned u) {
  return (float)__builtin_bit_cast(T, (uint16_t)(u & 0xffffu));
}
template <typename T>
__device__ __forceinline__ float hi_f(unsigned u) {
  return (float)__builtin_bit_cast(T, (uint16_t)(u >> 16));
}

struct XSet {
  uint4 x[KJ];   // A operand: input pixel channels 16j + 8*lh .. +8
};
struct ASet {
  uint2 a[16];   // skip / residual: channels 4*l32 .. +4 of the target of tile pixel 8(r/4) + r%4 + 4*lh
};
// LDS row of a phase's output channel co: MFMA column n of channel fragment i is channel 4n + i
__device__ __forceinline__ int wrow(int co) { return ((co & 3) << 5) | (co >> 2); }

// A workgroup owns NP consecutive phases of the s*s and a run of 32-pixel input tiles; per tile
// a wave loads the input operand once and runs the NP phases, the skip chunks of the next phase
// step in flight under the current one (NP = 4 on large inputs; NP = 1 spreads small inputs over
// s*s times more workgroups).
template <typename T, int NP>
__device__ __forceinline__ void convt_tile(const ConvTParams& p, const int bx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(NP == 1 || NP % 2 == 0, "phase group");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, lh = lane >> 5;
  const int group = __builtin_amdgcn_readfirstlane(bx / p.nchunks);  // (uniform: kept in scalar registers)
  const int chunk = bx - group * p.nchunks;
  const int phase0 = group * NP;

  // ---- the group's weights and bias into LDS (rows n = phase*C + co of the packed [N][Kpad])
  // (every load of the copy is issued before the first LDS write: one memory latency for the whole
  // prologue instead of one per 16-byte chunk, which serialised ~16 L2/HBM round trips per wave)
  {
    const char* wsrc = reinterpret_cast<const char*>(p.weight) + (size_t)phase0 * C * p.Kpad * sizeof(T);
    constexpr int NCH = NP * C * 16 / NT;  // 16-byte chunks per thread (NP * 4)
    static_assert((NP * C * 16) % NT == 0 && NP * C <= NT, "prologue split");
    uint4 wv[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * NT;
      const int r = i >> 4, c = i & 15;  // r = phase-in-group * C + co
      wv[k] = *reinterpret_cast<const uint4*>(wsrc + (size_t)r * p.Kpad * sizeof(T) + c * 16);
    }
    float* lb = reinterpret_cast<float*>(smem + NP * PW);
    const float bv = tid < NP * C ? p.bias[phase0 * C + tid] : 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * NT;
      const int r = i >> 4;
      *reinterpret_cast<uint4*>(smem + ((r & ~(C - 1)) + wrow(r & (C - 1))) * WPITCH + (i & 15) * 16) = wv[k];
    }
    if (tid < NP * C) lb[tid] = bv;
  }
  __syncthreads();

  // GEMM rows are input pixels (b, iy, ix)
  const int hw = p.h * p.w;
  const int M = p.B * hw;
  const int mt = (M + 31) / 32;
  // this wave's contiguous run of the group's tiles: an even split over all the group's waves
  // (every CU busy. Measured, profiles/convt_rows: a 32-frame 120x160 up-step moves 354 MB in
  // 0.064 ms = 5.5 TB/s, 0.88 of what a plain 16-byte-per-lane copy of the same footprint reaches
  // on the same machine (6.26 TB/s); with 32-byte pieces of 32 lines per instruction it was 4.0)
  const long long gw = (long long)chunk * NW + wave, nw = (long long)p.nchunks * NW;
  const int t_begin = (int)(mt * gw / nw);
  const int t_end = (int)(mt * (gw + 1) / nw);
  if (t_begin >= t_end) return;

  // the output as a buffer: rows of C channels at out_ldc, the last one ending the range
  const i32x4 orsrc = rsrc_of(p.out, (unsigned)(((size_t)(p.B * p.tH * p.tW - 1) * p.out_ldc + C) * sizeof(T)));
  // each phase's target offset (py + sy, px + sx): uniform, kept in scalar registers
  int oy[NP], ox[NP];
#pragma unroll
  for (int ph = 0; ph < NP; ++ph) {
    const int py = __builtin_amdgcn_readfirstlane((phase0 + ph) / p.s);
    oy[ph] = py + p.sy;
    ox[ph] = phase0 + ph - py * p.s + p.sx;
  }
  // target pixel index (b, Y, X) of this lane's pixel l32 in tile t for phase ph, or -1
  auto target = [&](int t, int ph) __attribute__((always_inline)) -> int {
    const int m = t * 32 + l32;
    if (m >= M) return -1;
    const int b = m / hw;
    const int rem = m - b * hw;
    const int iy = rem / p.w, ix = rem - iy * p.w;
    const int Y = iy * p.s + oy[ph], X = ix * p.s + ox[ph];
    if (Y >= p.tH || X >= p.tW) return -1;
    return (b * p.tH + Y) * p.tW + X;
  };
  // the target of tile pixel 8(r/4) + r%4 + 4*lh, the pixel of this lane's accumulator register r,
  // from the lane that computed it (two scalar lane reads and a select: no address registers)
  auto target_of = [&](int tg, int r) __attribute__((always_inline)) -> int {
    const int q = 8 * (r >> 2) + (r & 3);
    const int t0 = __builtin_amdgcn_readlane(tg, q), t1 = __builtin_amdgcn_readlane(tg, q + 4);
    return lh ? t1 : t0;
  };
  auto load_x = [&](int t, XSet& S) __attribute__((always_inline)) {
    const int m = t * 32 + l32;
    const size_t sp = (size_t)(m < M ? m : 0);
    const T* src = reinterpret_cast<const T*>(p.src) + sp * p.src_ldc + 8 * lh;
#pragma unroll
    for (int j = 0; j < KJ; ++j) S.x[j] = gload16(src + 16 * j);
  };
  // one instruction = the whole 256 B rows of two target pixels (phantom pixels read pixel 0)
  auto load_a = [&](int t, int ph, ASet& S) __attribute__((always_inline)) {
    const int tg = target(t, ph);
    const char* add = reinterpret_cast<const char*>(p.add);
    const unsigned pitch = (unsigned)p.add_ldc * (unsigned)sizeof(T);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = target_of(tg, r);
      S.a[r] = gload8(add + ((unsigned)(tr < 0 ? 0 : tr) * pitch + 8u * l32));  // (32-bit: launch checks the extent)
    }
  };

  auto compute_store = [&](int t, int ph, const XSet& X, const ASet& A) __attribute__((always_inline)) {
    const char* wl = smem + ph * PW + l32 * WPITCH + lh * 16;
    const f32x4 bb = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem + NP * PW) + ph * C + 4 * l32);
    const int tg = target(t, ph);
    const unsigned opitch = (unsigned)p.out_ldc * (unsigned)sizeof(T);
    // two halves of two channel fragments: half the accumulators live at a time (the x operand is
    // reused) — keeps the kernel inside 256 VGPRs without spills. The first half's result waits
    // as packed pairs, in the registers its skip words leave free, for the second half's store.
    unsigned o[2][16];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      f32x16 acc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] = f32x16{};
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        uint4 wv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) wv[i] = *reinterpret_cast<const uint4*>(wl + (2 * hf + i) * 32 * WPITCH + j * 32);
#pragma unroll
        for (int i = 0; i < 2; ++i) Mfma<T>::run(X.x[j], wv[i], acc[i]);
        __builtin_amdgcn_sched_barrier(0);
      }
      // register r: fragment i = channel 4*l32 + i of one pixel per lane half
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned sk = hf ? A.a[r].y : A.a[r].x;
        o[hf][r] = pack2<T>(lo_f<T>(sk) + (acc[0][r] + bb[2 * hf]), hi_f<T>(sk) + (acc[1][r] + bb[2 * hf + 1]));
        if (hf) {
          // (a range-checked buffer store: pixels with no target go past the range and are dropped,
          // so no store sits behind a branch)
          const int tr = target_of(tg, r);
          raw_buffer_store_v2(u32x2{o[0][r], o[1][r]}, orsrc, tr < 0 ? OOB : (int)((unsigned)tr * opitch + 8u * l32), 0, 0);
        }
      }
    }
  };

  // Steps (tile, phase) in order; the operands of the next step are loaded before the current
  // step's stores are issued (vector memory completes in issue order). Register sets
  // alternate: x by tile parity, skip by step parity (NP is 1 or even) -> unrolled by 2 tiles.
  XSet x0, x1;
  ASet a0, a1;
  load_x(t_begin, x0);
  load_a(t_begin, 0, a0);
  if constexpr (NP == 1) {
    // single phase: both sets alternate per tile
    for (int t = t_begin; t < t_end; t += 2) {
      if (t + 1 < t_end) {
        load_x(t + 1, x1);
        load_a(t + 1, 0, a1);
      }
      compute_store(t, 0, x0, a0);
      if (t + 1 >= t_end) break;
      if (t + 2 < t_end) {
        load_x(t + 2, x0);
        load_a(t + 2, 0, a0);
      }
      compute_store(t + 1, 0, x1, a1);
    }
  } else {
    // NP (even) phases per tile: skip sets alternate per phase (even phases a0), x per tile
    auto tile = [&](int t, XSet& xc, XSet& xn) __attribute__((always_inline)) {
#pragma unroll
      for (int ph = 0; ph < NP; ph += 2) {
        load_a(t, ph + 1, a1);
        compute_store(t, ph, xc, a0);
        __builtin_amdgcn_sched_barrier(0);
        if (ph + 2 < NP) {
          load_a(t, ph + 2, a0);
        } else if (t + 1 < t_end) {
          load_x(t + 1, xn);
          load_a(t + 1, 0, a0);
        }
        compute_store(t, ph + 1, xc, a1);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    for (int t = t_begin; t < t_end; t += 2) {
      tile(t, x0, x1);
      if (t + 1 >= t_end) break;
      tile(t + 1, x1, x0);
    }
  }
}

template <typename T, int NP>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT), amdgpu_waves_per_eu(2, 2))) void convt_add(ConvTParams p) {
  convt_tile<T, NP>(p, blockIdx.x);
}

// several independent up-steps in one launch (the engine's schedule: ops of one dependency level
// on the latency path): workgroups [end[k-1], end[k]) run up-step k
struct ConvTGroup {
  ConvTParams p[kConvTGroupMax];
  int end[kConvTGroupMax];
  int n;
};
template <typename T, int NP>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT), amdgpu_waves_per_eu(2, 2))) void convt_add_group(
    const ConvTGroup g) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < g.n && b >= g.end[k]) ++k;  // (workgroup-uniform)
  convt_tile<T, NP>(g.p[k], b - (k ? g.end[k - 1] : 0));
}

template <typename T, int NP>
static int launch_group_t(const ConvTGroup& g, hipStream_t s) {
  constexpr int lds = lds_bytes<NP>();
  if (int r = ensure_lds<convt_add_group<T, NP>>(lds)) return r;
  auto k = convt_add_group<T, NP>;
  hipLaunchKernelGGL(k, dim3(g.end[g.n - 1]), dim3(NT), lds, s, g);
  TV_HIP(hipGetLastError());
  return 0;
}

template <typename T, int NP>
static int launch_t(const ConvTParams& p, hipStream_t s) {
  auto k = convt_add<T, NP>;
  constexpr int lds = lds_bytes<NP>();
  if (int r = ensure_lds<convt_add<T, NP>>(lds)) return r;
  const int groups = p.s * p.s / NP;
  hipLaunchKernelGGL(k, dim3(groups * p.nchunks), dim3(NT), lds, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace convt

bool convt_supported(int cin, int cout, int src_ldc, int add_ldc, int out_ldc) {
  return cin == convt::KJ * 16 && cout == convt::C && src_ldc % 8 == 0 && add_ldc % 8 == 0 && out_ldc % 8 == 0;
}

// one resident 8-wave workgroup per CU over the whole launch, the tiles split evenly over the
// waves of each phase group (round-2 schedule: whole tiles-per-wave counts, which left 56 of 256
// CUs idle on the 120x160 up-steps)
void convt_schedule(ConvTParams& p, int cu_count) {
  const long M = (long)p.B * p.h * p.w;
  const long mt = (M + 31) / 32;
  const long waves_target = (long)convt::NW * cu_count;
  // phase groups of 4 once every wave of the launch gets >= 2 tiles that way
  p.np = (p.s * p.s % convt::NPG == 0 &&
          mt * (p.s * p.s / convt::NPG) >= 2 * waves_target) ? convt::NPG : 1;
  const long groups = (long)p.s * p.s / p.np;
  long chunks = cu_count / groups;                       // workgroups per phase group
  const long need = (mt + convt::NW - 1) / convt::NW;    // no more than one tile per wave's worth
  if (chunks > need) chunks = need;
  if (chunks < 1) chunks = 1;
  p.nchunks = (int)chunks;
  p.tpw = (int)((mt + chunks * convt::NW - 1) / (chunks * convt::NW));  // most tiles any wave runs
}

// the kernel addresses the skip and output rows with 32-bit byte offsets
static bool convt_fits(const ConvTParams& p) {
  const long long rows = (long long)p.B * p.tH * p.tW;
  const long long ldc = std::max(p.add_ldc, p.out_ldc);
  return rows >= 1 && rows * ldc * 2 < (1ll << 31);
}

int convt_workgroups(const ConvTParams& p) { return p.s * p.s / std::max(1, p.np) * p.nchunks; }

int launch_convt_group(const ConvTParams* const* ps, int n, int dtype, hipStream_t s) {
  using namespace convt;
  if (n < 1 || n > kConvTGroupMax) {
    set_error("convt group: 1..kConvTGroupMax up-steps");
    return 1;
  }
  ConvTGroup g{};
  g.n = n;
  int wg = 0;
  for (int k = 0; k < n; ++k) {
    const ConvTParams& p = *ps[k];
    if (p.tpw < 1 || p.nchunks < 1 || p.s < 1 || p.np != ps[0]->np || (p.np != 1 && p.np != NPG)) {
      set_error("convt group: unscheduled or mixed phase groups");
      return 1;
    }
    if (!convt_fits(p)) {
      set_error("convt: target tensor of 2 GiB or more");
      return 1;
    }
    wg += convt_workgroups(p);
    g.p[k] = p;
    g.end[k] = wg;
  }
  const bool np4 = ps[0]->np == NPG;
  if (dtype == F16) return np4 ? launch_group_t<_Float16, NPG>(g, s) : launch_group_t<_Float16, 1>(g, s);
  if (dtype == BF16) return np4 ? launch_group_t<__bf16, NPG>(g, s) : launch_group_t<__bf16, 1>(g, s);
  set_error("convt: fp16/bf16 only");
  return 1;
}

int launch_convt(const ConvTParams& p, int dtype, hipStream_t s) {
  if (p.tpw < 1 || p.nchunks < 1 || p.s < 1) {
    set_error("convt: not scheduled");
    return 1;
  }
  using namespace convt;
  if (!convt_fits(p)) {
    set_error("convt: target tensor of 2 GiB or more");
    return 1;
  }
  if (p.np != 1 && p.np != NPG) {
    set_error("convt: bad phase group");
    return 1;
  }
  if (dtype == F16) return p.np == NPG ? launch_t<_Float16, NPG>(p, s) : launch_t<_Float16, 1>(p, s);
  if (dtype == BF16) return p.np == NPG ? launch_t<__bf16, NPG>(p, s) : launch_t<__bf16, 1>(p, s);
  set_error("convt: fp16/bf16 only");
  return 1;
}

}  // namespace tv
