// YOLACT evaluation on the device: the pixel counts behind the mask IoU, and the detection-to-truth
// matching for box and mask average precision at T IoU thresholds (contracts: tv_yolact_mask_overlap and
// tv_yolact_evaluate_match in include/tauv_vision_amd.h).
//
// overlap. The detections' masks arrive as packed bits (tv_yolact_frame_masks' layout) and the truths as
// ONE seg map in which pixel value t means truth t, so the truth masks are disjoint and the K x N
// intersections are one pass over the seg map. A workgroup owns one image and a band of kBand rows. Lane
// j of a wave is the keeper of detection g * 64 + j (g: the wave's keeper group, ceil(K / 64) of them);
// where the groups leave waves over, they split the band's rows. Per 64-pixel strip a wave reads the 64
// seg bytes, one per lane, and peels the distinct owners with readlane + ballot into wave-uniform
// 64-bit masks (typically one to three per strip; 64 when every pixel has another owner); the valid-pixel
// mask is a ballot too. Each keeper adds popcount(own word & mask) to its column of the wave's own LDS
// table [N][64]: lanes are consecutive, so no bank conflict and no LDS atomic. A keeper's words of one
// frame row are contiguous: with ceil(W / 32) a multiple of 4 they are fetched 16 B at a time (two
// strips), else word by word. det_area stays in a register per keeper, truth_area in lane t of the
// waves of group 0. At the end the waves add their non-zero entries to the outputs with integer global
// atomics (exact in any order); a zeroing launch goes in front.
//
// match. One workgroup of four waves per image. All threads derive every record's label and score from
// its softmax row and its walk rank from the scores (the records need not be sorted). Then wave w walks
// the records in rank order for kind w & 1 (0 box, 1 mask) and its half of the thresholds; lane t holds
// truth t, forms its IoU with the current detection on the fly, and keeps one free bit per threshold.
// Per threshold the candidates are a ballot; none or one (the usual cases) is settled there, more are
// compared through readlane in ascending truth index (strictly larger IoU replaces: the lowest index
// wins a tie). The results go through LDS and leave as det_truth and the log rows of the batch.
#include "common.h"
#include "yolact_eval_dev.h"

namespace tv {
namespace yeval {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBand = 8;  // frame rows per workgroup of the overlap pass
constexpr int kMaxK = 256;
constexpr int kMaxN = 64;
constexpr int kMaxT = 16;
constexpr int kMaxC = 254;
constexpr int kInvalidPixel = 254;

struct OverlapParams {
  const uint32_t* bits;       // [B][K][H][ww]
  const int* counts;          // [B]
  const uint8_t* seg;         // [B][H][W]
  const uint8_t* truth_valid; // [B][N]
  int B, K, N, H, W;
  int wc, ww;                 // strips per row ceil(W / 64), words per row ceil(W / 32)
  int vec;                    // ww % 4 == 0 and `bits` 16-B aligned: a keeper's row is whole aligned 16-B pieces
  int* inter;                 // [B][K][N]
  int* det_area;              // [B][K]
  int* truth_area;            // [B][N]
};

__global__ __launch_bounds__(kThreads) void zero_counts(int* inter, long long n_inter, int* det_area, long long n_det,
                                                        int* truth_area, long long n_truth) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_inter) inter[i] = 0;
  else if (i < n_inter + n_det) det_area[i - n_inter] = 0;
  else if (i < n_inter + n_det + n_truth) truth_area[i - n_inter - n_det] = 0;
}

// One strip: `word` is the keeper's 64 pixels, `v` the lane's seg byte.
__device__ __forceinline__ void strip(unsigned long long word, int v, bool inside, unsigned long long tv_mask, int N,
                                      int lane, int* tbl, int& area, int& t_area) {
  const bool valid = inside && v != kInvalidPixel;
  const bool owned = valid && v < N && ((tv_mask >> (v & 63)) & 1ull);
  area += (int)__popcll(word & __ballot(valid));
  unsigned long long pending = __ballot(owned);
  while (pending) {
    const int t = __builtin_amdgcn_readlane(v, (int)__builtin_ctzll(pending));  // < N: its lane is `owned`
    const unsigned long long m = __ballot(owned && v == t);
    pending &= ~m;
    const int c = (int)__popcll(word & m);
    if (c) tbl[t * 64 + lane] += c;
    if (lane == t) t_area += (int)__popcll(m);
  }
}

__global__ __launch_bounds__(kThreads) void overlap(const OverlapParams p) {
  extern __shared__ int s_tbl[];  // [kWaves][N][64]
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y;
  const int K = p.K, N = p.N, H = p.H, W = p.W, ww = p.ww;
  const int kg = (K + 63) >> 6;       // keeper groups, 1..4
  const int nsub = kWaves / kg;       // waves per group: they split the band's rows
  const int g = wave % kg, r = wave / kg;
  if (r >= nsub) return;              // (kg == 3: the fourth wave has no work; the kernel has no barrier)
  int* tbl = s_tbl + wave * N * 64;
  for (int t = 0; t < N; ++t) tbl[t * 64 + lane] = 0;

  const int cnt = min(max(p.counts[b], 0), K);
  const int d = g * 64 + lane;
  const bool keeper = d < cnt;        // rows at or past counts[b] are not read
  unsigned long long tv_mask = __ballot(lane < N && p.truth_valid[(size_t)b * N + min(lane, N - 1)] != 0);
  const bool vec = p.vec != 0;
  int area = 0, t_area = 0;
  const int y_end = min((int)(blockIdx.x + 1) * kBand, H);
  for (int y = blockIdx.x * kBand + r; y < y_end; y += nsub) {
    const uint8_t* srow = p.seg + ((size_t)b * H + y) * W;
    const uint32_t* brow = p.bits + (((size_t)b * K + min(d, K - 1)) * H + y) * ww;
    for (int s0 = 0; s0 < p.wc; s0 += 2) {  // two strips = four words
      uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
      if (keeper) {
        if (vec) {
          const uint4 q = *reinterpret_cast<const uint4*>(brow + 2 * s0);
          w0 = q.x; w1 = q.y; w2 = q.z; w3 = q.w;
        } else {
          const int a = 2 * s0;
          w0 = brow[a];
          if (a + 1 < ww) w1 = brow[a + 1];
          if (a + 2 < ww) w2 = brow[a + 2];
          if (a + 3 < ww) w3 = brow[a + 3];
        }
      }
      const int xa = s0 * 64 + lane, xb = xa + 64;
      const int va = xa < W ? (int)srow[xa] : kInvalidPixel;
      const int vb = xb < W ? (int)srow[xb] : kInvalidPixel;
      strip(((unsigned long long)w1 << 32) | w0, va, xa < W, tv_mask, N, lane, tbl, area, t_area);
      if (s0 + 1 < p.wc) strip(((unsigned long long)w3 << 32) | w2, vb, xb < W, tv_mask, N, lane, tbl, area, t_area);
    }
  }
  if (keeper) {
    if (area) atomicAdd(p.det_area + (size_t)b * K + d, area);
    int* out = p.inter + ((size_t)b * K + d) * N;
    for (int t = 0; t < N; ++t) {
      const int c = tbl[t * 64 + lane];
      if (c) atomicAdd(out + t, c);
    }
  }
  if (g == 0 && lane < N && t_area) atomicAdd(p.truth_area + (size_t)b * N + lane, t_area);
}

struct MatchParams {
  const float* confidence;    // [B][K][C + 1]
  const float* records;       // [B][K][8]
  const int* counts;          // [B]
  const uint8_t* truth_valid; // [B][N]
  const long long* truth_label;  // [B][N]
  const float* truth_box;     // [B][N][4] y, x, h, w
  const int* inter;           // [B][K][N]
  const int* det_area;        // [B][K]
  const int* truth_area;      // [B][N]
  const float* thr;           // [T]
  int B, K, N, C, T;
  const long long* cursor;    // [1]
  int* log;                   // [capacity][K][4]
  long long capacity;
  int* det_truth;             // [B][K][2][T]
  unsigned long long* totals; // [C + 2]
};

__global__ __launch_bounds__(kThreads) void match(const MatchParams p) {
  __shared__ float s_score[kMaxK];
  __shared__ unsigned s_key[kMaxK];
  __shared__ int s_label[kMaxK];
  __shared__ unsigned short s_order[kMaxK];        // rank -> record
  __shared__ signed char s_dt[kMaxK * 2 * kMaxT];  // [record][kind][threshold]
  __shared__ unsigned s_tp[kWaves][kMaxK];         // the tp bits a wave found, by record
  __shared__ float s_box[kMaxK][4];
  __shared__ int s_darea[kMaxK];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = p.K, N = p.N, C = p.C, T = p.T;
  const int n = min(max(p.counts[b], 0), K);

  for (int i = tid; i < K; i += kThreads) {
    int label = 0;
    float score = 0.f;
    if (i < n) label_score(p.confidence + ((size_t)b * K + i) * (C + 1), C, &label, &score);
    s_label[i] = label;
    s_score[i] = score;
    s_key[i] = score_key(score);
    s_darea[i] = p.det_area[(size_t)b * K + i];
    for (int c = 0; c < 4; ++c) s_box[i][c] = p.records[((size_t)b * K + i) * 8 + 4 + c];
    for (int w = 0; w < kWaves; ++w) s_tp[w][i] = 0u;
  }
  for (int i = tid; i < K * 2 * T; i += kThreads) s_dt[i] = -1;
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const unsigned ki = s_key[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += walks_before(s_key[j], j, ki, i) ? 1 : 0;
    s_order[rank] = (unsigned short)i;  // the ranks are a permutation of 0 .. n-1
  }
  __syncthreads();

  // the walk: kind and threshold range of this wave, truth `lane`
  {
    const int kind = wave & 1;
    const int half = (T + 1) >> 1;
    const int j0 = (wave >> 1) * half, j1 = min(j0 + half, T);
    const bool have = lane < N;
    const size_t g = (size_t)b * N + (have ? lane : 0);
    const long long t_label = p.truth_label[g];
    const bool t_ok = have && p.truth_valid[g] != 0 && t_label >= 1 && t_label <= (long long)C;
    const float ty = p.truth_box[g * 4 + 0], tx = p.truth_box[g * 4 + 1], th = p.truth_box[g * 4 + 2],
                tw = p.truth_box[g * 4 + 3];
    const int t_area = p.truth_area[g];
    const double tau = (lane >= j0 && lane < j1) ? (double)p.thr[lane] : 0.0;  // lane j holds threshold j
    unsigned free_bits = 0xFFFFu;  // bit j: this truth is still free at threshold j
    const int* inter_b = p.inter + (size_t)b * K * N;
    int nxt = (kind == 1 && n > 0 && have) ? inter_b[(size_t)s_order[0] * N + lane] : 0;
    for (int r = 0; r < n && j0 < j1; ++r) {
      const int i = s_order[r];
      const int in = nxt;
      if (kind == 1 && r + 1 < n && have) nxt = inter_b[(size_t)s_order[r + 1] * N + lane];  // one record ahead
      const bool same = t_ok && t_label == (long long)s_label[i];
      double iou = 0.0;
      if (same) {
        if (kind == 0) {
          iou = box_iou(s_box[i][0], s_box[i][1], s_box[i][2], s_box[i][3], ty, tx, th, tw);
        } else {
          iou = mask_iou(in, s_darea[i], t_area);
        }
      }
      if (__ballot(same) == 0ull) continue;  // no truth of this label: every entry stays -1
      const int lo = (int)__double2loint(iou), hi = (int)__double2hiint(iou);
      int mine = -1;  // lane j: the truth taken at threshold j
      for (int j = j0; j < j1; ++j) {
        const double tj = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(tau), j),
                                           __builtin_amdgcn_readlane(__double2loint(tau), j));
        unsigned long long cand = __ballot(same && ((free_bits >> j) & 1u) && iou >= tj);
        if (cand == 0ull) continue;
        int best = (int)__builtin_ctzll(cand);
        cand &= cand - 1;
        if (cand) {
          double bi = __hiloint2double(__builtin_amdgcn_readlane(hi, best), __builtin_amdgcn_readlane(lo, best));
          while (cand) {
            const int u = (int)__builtin_ctzll(cand);
            cand &= cand - 1;
            const double ui = __hiloint2double(__builtin_amdgcn_readlane(hi, u), __builtin_amdgcn_readlane(lo, u));
            if (ui > bi) { bi = ui; best = u; }
          }
        }
        if (lane == best) free_bits &= ~(1u << j);
        if (lane == j) mine = best;
      }
      const unsigned long long hit = __ballot(mine >= 0);  // bits j0 .. j1-1
      if (lane >= j0 && lane < j1) s_dt[(i * 2 + kind) * T + lane] = (signed char)mine;
      if (lane == 0) s_tp[wave][i] = (unsigned)hit << (16 * kind);
    }
  }
  __syncthreads();

  int* dt = p.det_truth + (size_t)b * K * 2 * T;
  for (int i = tid; i < K * 2 * T; i += kThreads) dt[i] = (int)s_dt[i];
  const long long row = p.cursor[0] + b;
  if (row >= 0 && row < p.capacity) {
    int4* log = reinterpret_cast<int4*>(p.log) + (size_t)row * K;
    for (int i = tid; i < K; i += kThreads) {
      int4 q = make_int4(0, 0, 0, 0);
      if (i < n) {
        q.x = __float_as_int(s_score[i]);
        q.y = s_label[i];
        q.z = (int)(s_tp[0][i] | s_tp[1][i] | s_tp[2][i] | s_tp[3][i]);
        q.w = 1;
      }
      log[i] = q;
    }
  }
  if (tid < N) {
    const size_t g = (size_t)b * N + tid;
    if (p.truth_valid[g] != 0) {
      const long long l = p.truth_label[g];
      atomicAdd(p.totals + ((l >= 1 && l <= (long long)C) ? (int)l : C + 1), 1ull);
    }
  }
}

__global__ void advance_cursor(long long* cursor, long long by) { cursor[0] += by; }

}  // namespace yeval

int launch_yolact_mask_overlap(const uint32_t* bits, const int* counts, const uint8_t* seg, const uint8_t* truth_valid,
                               int B, int K, int N, int H, int W, int* inter, int* det_area, int* truth_area,
                               hipStream_t s) {
  using namespace yeval;
  if (!bits || !counts || !seg || !truth_valid || !inter || !det_area || !truth_area) {
    set_error("yolact_mask_overlap: null pointer");
    return 1;
  }
  if (B < 1) { set_error("yolact_mask_overlap: B must be >= 1"); return 1; }
  if (K < 1 || K > kMaxK) { set_error("yolact_mask_overlap: K must be in 1..256"); return 1; }
  if (N < 1 || N > kMaxN) { set_error("yolact_mask_overlap: N must be in 1..64"); return 1; }
  if (H < 1 || W < 1) { set_error("yolact_mask_overlap: H and W must be >= 1"); return 1; }
  if (W > (1 << 30) || B > 65535) { set_error("yolact_mask_overlap: W <= 2^30 and B <= 65535"); return 1; }
  if ((long long)H * W > 0x7FFFFFFFLL) { set_error("yolact_mask_overlap: H * W exceeds the int32 counts"); return 1; }
  OverlapParams p{};
  p.bits = bits; p.counts = counts; p.seg = seg; p.truth_valid = truth_valid;
  p.B = B; p.K = K; p.N = N; p.H = H; p.W = W; p.wc = (W + 63) / 64; p.ww = (W + 31) / 32;
  p.vec = (p.ww % 4 == 0 && (reinterpret_cast<uintptr_t>(bits) & 15u) == 0) ? 1 : 0;
  p.inter = inter; p.det_area = det_area; p.truth_area = truth_area;
  const long long n_inter = (long long)B * K * N, n_det = (long long)B * K, n_truth = (long long)B * N;
  const long long total = n_inter + n_det + n_truth;
  hipLaunchKernelGGL(zero_counts, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, inter,
                     n_inter, det_area, n_det, truth_area, n_truth);
  TV_HIP(hipGetLastError());
  const size_t lds = (size_t)kWaves * N * 64 * sizeof(int);  // <= 64 KiB
  hipLaunchKernelGGL(overlap, dim3((unsigned)((H + kBand - 1) / kBand), (unsigned)B), dim3(kThreads), lds, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_yolact_evaluate_match(const float* confidence, const float* records, const int* counts,
                                 const uint8_t* truth_valid, const long long* truth_label, const float* truth_box,
                                 const int* inter, const int* det_area, const int* truth_area,
                                 const float* iou_thresholds, int B, int K, int N, int C, int T, long long* cursor,
                                 int* log, long long capacity, int* det_truth, long long* totals, hipStream_t s) {
  using namespace yeval;
  if (!confidence || !records || !counts || !truth_valid || !truth_label || !truth_box || !inter || !det_area ||
      !truth_area || !iou_thresholds || !cursor || !log || !det_truth || !totals) {
    set_error("yolact_evaluate_match: null pointer");
    return 1;
  }
  if (B < 1) { set_error("yolact_evaluate_match: B must be >= 1"); return 1; }
  if (K < 1 || K > kMaxK) { set_error("yolact_evaluate_match: K must be in 1..256"); return 1; }
  if (N < 1 || N > kMaxN) { set_error("yolact_evaluate_match: N must be in 1..64"); return 1; }
  if (C < 1 || C > kMaxC) { set_error("yolact_evaluate_match: C must be in 1..254"); return 1; }
  if (T < 1 || T > kMaxT) { set_error("yolact_evaluate_match: T must be in 1..16"); return 1; }
  if (capacity < 0) { set_error("yolact_evaluate_match: negative log capacity"); return 1; }
  if (reinterpret_cast<uintptr_t>(log) & 15u) { set_error("yolact_evaluate_match: the log must be 16-byte aligned"); return 1; }
  MatchParams p{};
  p.confidence = confidence; p.records = records; p.counts = counts; p.truth_valid = truth_valid;
  p.truth_label = truth_label; p.truth_box = truth_box; p.inter = inter; p.det_area = det_area;
  p.truth_area = truth_area; p.thr = iou_thresholds; p.B = B; p.K = K; p.N = N; p.C = C; p.T = T;
  p.cursor = cursor; p.log = log; p.capacity = capacity; p.det_truth = det_truth;
  p.totals = (unsigned long long*)totals;
  hipLaunchKernelGGL(match, dim3((unsigned)B), dim3(kThreads), 0, s, p);
  TV_HIP(hipGetLastError());
  hipLaunchKernelGGL(advance_cursor, dim3(1), dim3(1), 0, s, cursor, (long long)B);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
