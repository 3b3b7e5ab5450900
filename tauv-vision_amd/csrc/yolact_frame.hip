// YOLACT instance masks at the size of the camera frame: what both reference callers do with the
// assembled masks [B, n, mh, mw] after assemble_mask.
//   evaluate_batch.py:98-102   F.interpolate(mask, (in_h, in_w), mode="bilinear"), mask > 0.5
//   yolact_node.py:135,143,184 F.interpolate(mask, (H_raw, W_raw)) (nearest), mask_np > 0.5
//   utils/plot.py:148-152      per detection, in order: img[mask] = 0.5 colour + 0.5 img[mask] on the
//                              uint8 frame (restated in evaluate_batch.py:136-139)
// The up-sampled fp32 mask is never stored. Each wave owns 64 consecutive frame columns of one frame
// row; a lane keeps its column's source taps and weights (and, for the overlay, its pixel's three
// channels) in registers over all detections. Detections are taken 64 at a time, and in a group lane
// j is also the keeper of detection base + j:
//   * it decides whether the wave evaluates that detection at all (d < counts[b], and with
//     bound_by_box its box crop reaches the wave's row and columns) and, for the overlay, fetches its
//     colour; the ballot of the decisions is the wave's work list;
//   * the wave walks the list in ascending d (the blend order), kFan detections per step so that their
//     mask loads are in flight together: every lane evaluates its pixel's up-sampled value, `> 0.5`
//     goes through a ballot, the 64 bits land in the keeper lane's registers, the overlay lanes blend;
//   * after the walk each keeper stores its detection's two 32-bit words — zeros for a detection that
//     was not on the list — and adds the popcount to its area (an integer atomic: exact in any order;
//     none where the count is 0). One store instruction and one atomic instruction per 64
//     detections: on gfx950 stores and atomics retire through the same counter as loads, in order, so
//     a store per detection inside the walk made every step wait for the previous step's write.
// So every word of `bits` is written by every call, and the masks are read only inside their crops.
// The assembled masks are small (n mh mw floats per frame) and each source row is re-read by H / mh
// frame rows from cache; the streams that reach HBM are the frame, the overlay and the bits. `area`
// is zeroed by a launch of its own in front (stream order).
#include "common.h"
#include "resample_dev.h"

namespace tv {
namespace frame {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFan = 4;  // detections evaluated per step of the walk

struct Params {
  const float* masks;    // [B][n][mh][mw]
  int mh, mw;
  const int* counts;     // [B]
  int B, n, H, W;
  int wc, ww;            // waves per row ceil(W / 64), words per row ceil(W / 32)
  long long units;       // B * H * wc waves of work
  float sh, sw;          // (float)mh / (float)H, (float)mw / (float)W
  int bound_by_box;
  const long long* det;  // [B][n] row of `box` per detection
  const float* box;      // [B][A][4] y, x, h, w
  int A;
  const uint8_t* frames;   // [B][H][W][3] or null
  const float* records;    // [B][n][8], class id in column 1
  const uint8_t* palette;  // [n_colours][3]
  int n_colours;
  uint32_t* bits;        // [B][n][H][ww]
  int* area;             // [B][n]
  uint8_t* overlay;      // [B][H][W][3]
};

__global__ __launch_bounds__(kThreads) void zero_area(int* area, int total) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < total) area[i] = 0;
}

template <bool BILINEAR, bool OVERLAY>
__global__ __launch_bounds__(kThreads) void frame_masks(const Params p) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long long unit = (long long)blockIdx.x * kWaves + wave;
  if (unit >= p.units) return;  // whole waves; the kernel has no barrier
  const int chunk = (int)(unit % p.wc);
  const long long by = unit / p.wc;
  const int y = (int)(by % p.H), b = (int)(by / p.H);
  const int xa = chunk * 64, x = xa + lane;
  const bool inside = x < p.W;
  const int xc = min(x, p.W - 1);  // lanes past the row end compute on its last pixel and select nothing
  const int cnt = min(max(p.counts[b], 0), p.n);

  // the lane's source offsets (and weights) inside one mask: the same for every detection
  int o00, o01 = 0, o10 = 0, o11 = 0;
  float h0 = 0.f, h1 = 0.f, w0 = 0.f, w1 = 0.f;
  if (BILINEAR) {
    int y0, y1, x0, x1;
    resample::lin_index(y, p.mh, p.sh, y0, y1, h0, h1);
    resample::lin_index(xc, p.mw, p.sw, x0, x1, w0, w1);
    o00 = y0 * p.mw + x0;
    o01 = y0 * p.mw + x1;
    o10 = y1 * p.mw + x0;
    o11 = y1 * p.mw + x1;
  } else {
    o00 = resample::nearest_src(y, p.sh, p.mh) * p.mw + resample::nearest_src(xc, p.sw, p.mw);
  }

  const size_t pixel = (((size_t)b * p.H + y) * p.W + xc) * 3;
  int c0 = 0, c1 = 0, c2 = 0;
  if (OVERLAY) {
    c0 = p.frames[pixel];
    c1 = p.frames[pixel + 1];
    c2 = p.frames[pixel + 2];
  }
  const size_t mask_px = (size_t)p.mh * p.mw;
  const size_t row_words = (size_t)p.H * p.ww;             // words per detection
  const size_t word0 = (size_t)y * p.ww + 2 * (size_t)chunk;  // the wave's first word inside a detection
  const bool two = 2 * chunk + 1 < p.ww;                   // the row's last wave may own one word only

  for (int base = 0; base < p.n; base += 64) {
    const int dl = base + lane;  // the detection this lane keeps
    bool hit = dl < cnt;
    unsigned colour = 0;
    if (hit) {
      const size_t bd = (size_t)b * p.n + dl;
      if (p.bound_by_box) {
        const long long a = p.det[bd];
        if (a >= 0 && a < p.A) {  // (not a row of `box`: nothing to bound by, the wave evaluates it)
          int bx0, bx1, by0, by1;
          resample::box_crop(p.box + ((size_t)b * p.A + (size_t)a) * 4, p.mh, p.mw, p.H, p.W, BILINEAR ? 1.f : 0.f,
                             bx0, bx1, by0, by1);
          hit = y >= by0 && y <= by1 && bx1 >= xa && bx0 <= xa + 63;
        }
      }
      if (OVERLAY && hit) {
        const float cf = p.records[bd * 8 + 1];
        const int cls = cf >= 0.f ? (int)fminf(cf, (float)(p.n_colours - 1)) : 0;  // (a NaN id: colour 0)
        const uint8_t* col = p.palette + (size_t)cls * 3;
        colour = (unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16);
      }
    }
    unsigned long long todo = __ballot(hit);
    unsigned long long mine = 0;  // the 64 pixels of detection dl
    while (todo) {  // ascending d: the blend order of the reference's loop
      int j[kFan];
      bool live[kFan];
      float v[kFan];
#pragma unroll
      for (int u = 0; u < kFan; ++u) {
        live[u] = todo != 0;
        j[u] = live[u] ? __builtin_ctzll(todo) : j[0];  // (a spent slot re-reads slot 0's mask: no branch around a load)
        todo &= todo - 1;
      }
#pragma unroll
      for (int u = 0; u < kFan; ++u) {
        const float* m = p.masks + ((size_t)b * p.n + (base + j[u])) * mask_px;
        if (BILINEAR) v[u] = resample::lin_blend(m[o00], m[o01], m[o10], m[o11], h0, h1, w0, w1);
        else v[u] = m[o00];
      }
#pragma unroll
      for (int u = 0; u < kFan; ++u) {
        const bool sel = live[u] && inside && v[u] > 0.5f;
        const unsigned long long bal = __ballot(sel);
        if (lane == j[u] && live[u]) mine = bal;
        if (OVERLAY) {
          const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)colour, j[u]);
          if (sel) {
            c0 = (c0 + (int)(k & 255u)) >> 1;
            c1 = (c1 + (int)((k >> 8) & 255u)) >> 1;
            c2 = (c2 + (int)(k >> 16)) >> 1;
          }
        }
      }
    }
    if (dl < p.n) {
      const size_t bd = (size_t)b * p.n + dl;
      uint32_t* w = p.bits + bd * row_words + word0;
      w[0] = (uint32_t)mine;
      if (two) w[1] = (uint32_t)(mine >> 32);
      if (mine) atomicAdd(p.area + bd, (int)__popcll(mine));
    }
  }
  if (OVERLAY && inside) {
    p.overlay[pixel] = (uint8_t)c0;
    p.overlay[pixel + 1] = (uint8_t)c1;
    p.overlay[pixel + 2] = (uint8_t)c2;
  }
}

}  // namespace frame

int launch_yolact_frame_masks(const float* masks, int mh, int mw, const int* counts, int B, int n, int H, int W, int mode,
                              int bound_by_box, const long long* det, const float* box, int A, const uint8_t* frames,
                              const float* records, const uint8_t* palette, int n_colours, uint32_t* bits, int* area,
                              uint8_t* overlay, hipStream_t s) {
  if (B < 0 || n < 0) { set_error("frame_masks: negative B or n"); return 1; }
  if ((long long)B * n == 0) return 0;
  if (!masks || !counts || !bits || !area) { set_error("frame_masks: null pointer"); return 1; }
  if (mh < 1 || mw < 1 || H < 1 || W < 1) { set_error("frame_masks: mask and frame sizes must be positive"); return 1; }
  if (mode != 0 && mode != 1) { set_error("frame_masks: mode must be 0 (bilinear) or 1 (nearest)"); return 1; }
  if (bound_by_box && (!det || !box || A < 1)) { set_error("frame_masks: bound_by_box needs det, box and A >= 1"); return 1; }
  if ((frames == nullptr) != (overlay == nullptr)) { set_error("frame_masks: frames and overlay go together"); return 1; }
  if (frames && (!records || !palette)) { set_error("frame_masks: frames need records and palette"); return 1; }
  if (frames && n_colours < 1) { set_error("frame_masks: n_colours must be >= 1"); return 1; }
  if ((long long)mh * mw > 0x7FFFFFFFLL) { set_error("frame_masks: mask too large"); return 1; }
  if (W > (1 << 30) || (long long)B * n > 0x7FFFFFFFLL) { set_error("frame_masks: sizes exceed the index range"); return 1; }
  frame::Params p{};
  p.masks = masks; p.mh = mh; p.mw = mw; p.counts = counts; p.B = B; p.n = n; p.H = H; p.W = W;
  p.wc = (W + 63) / 64; p.ww = (W + 31) / 32;
  p.units = (long long)B * H * p.wc;
  p.sh = (float)mh / (float)H; p.sw = (float)mw / (float)W;
  p.bound_by_box = bound_by_box ? 1 : 0; p.det = det; p.box = box; p.A = A;
  p.frames = frames; p.records = records; p.palette = palette; p.n_colours = n_colours;
  p.bits = bits; p.area = area; p.overlay = overlay;
  const long long blocks = (p.units + frame::kWaves - 1) / frame::kWaves;
  if (blocks > 0x7FFFFFFFLL) { set_error("frame_masks: B * H * ceil(W / 64) exceeds the grid limit"); return 1; }
  const int total = B * n;
  hipLaunchKernelGGL(frame::zero_area, dim3((unsigned)((total + frame::kThreads - 1) / frame::kThreads)),
                     dim3(frame::kThreads), 0, s, area, total);
  TV_HIP(hipGetLastError());
  const dim3 grid((unsigned)blocks), block(frame::kThreads);
  if (mode == 0) {
    if (frames) hipLaunchKernelGGL((frame::frame_masks<true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((frame::frame_masks<true, false>), grid, block, 0, s, p);
  } else {
    if (frames) hipLaunchKernelGGL((frame::frame_masks<false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((frame::frame_masks<false, false>), grid, block, 0, s, p);
  }
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
