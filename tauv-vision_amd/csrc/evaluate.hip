// Detection-to-truth matching of the reference's evaluation scripts (centernet/scripts/evaluate.py:188-203,
// evaluate_keypoints.py:143-153) for B images in one launch, and the counts their precision / recall are
// made of, for T score thresholds at once. The reference walks the detections of an image in descending
// score (the later record first among equal scores: a stable sort, reversed); each takes the first truth
// still in the list, in truth order, that has its label and passes the match test, and that truth leaves
// the list. The detections at score threshold t are the records with score >= t, a prefix of that walk,
// so one walk over all the records gives every record its truth (or none) and n_tp(t), n_detections(t)
// are counts over score >= t.
//
// One workgroup of 256 threads per image.
//   a. All threads stage the scores (as sortable keys) and the truths in LDS and compute every record's
//      walk rank directly, #{j : s_j > s_i or (s_j == s_i and j > i)}: the records need not be sorted. A
//      NaN score has the lowest key (it walks last) and passes no threshold; the reference never has one.
//   b. All threads fill one 64-bit qualification word per (rank, 64 truths): a wave takes a record, its
//      lanes 64 truths, __ballot makes the word. Validity, the label test and the double arithmetic of
//      the match test are off the serial chain.
//   c. Wave 0 walks the ranks. Lane w holds word w of the free-truth mask (N <= 256: four lanes). Per
//      record: qual & free, the first lane with a bit left (ballot), its lowest bit, which that lane clears.
//   d. All threads store det_truth, and count per threshold the records with score >= t and the matched
//      ones among them (ballot + popcount), one atomic add per (image, threshold) and count, plus the
//      image's valid truths.
// The match tests are the reference's expressions in double on the fp32 values, uncontracted, in the
// order written there (its Python max / min / abs included).
#include "common.h"

namespace tv {
namespace evaluate {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;
constexpr int kMaxN = 256;
constexpr int kMaxT = 64;
constexpr int kWords = kMaxN / 64;  // words of the truth mask

struct Params {
  const float* records;  // [B][K][rec_stride]
  const int* counts;     // [B]
  int c_label, c_score, c_y, c_x, c_h, c_w;
  int rec_stride, K, N, T, mode;
  const uint8_t* t_valid;    // [B][N]
  const long long* t_label;  // [B][N]
  const float* t_center;     // [B][N][2]
  const float* t_size;       // [B][N][2]; may be null in centre mode
  double thr;
  const float* score_thr;  // [T]
  int* det_truth;          // [B][K]
  unsigned long long* totals;  // [2T + 1]
};

// Python's max(a, b) and min(a, b): the first argument unless the second is strictly beyond it.
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// evaluate.py:106-130 with d1 the detection and d2 the truth.
__device__ __forceinline__ bool box_pass(float y1, float x1, float h1, float w1, float y2, float x2, float h2, float w2,
                                         double thr) {
#pragma clang fp contract(off)
  const double Y1 = y1, X1 = x1, H1 = h1, W1 = w1, Y2 = y2, X2 = x2, H2 = h2, W2 = w2;
  const double ya = py_max(Y1 - H1 / 2, Y2 - H2 / 2);
  const double xa = py_max(X1 - W1 / 2, X2 - W2 / 2);
  const double yb = py_min(Y1 + H1 / 2, Y2 + H2 / 2);
  const double xb = py_min(X1 + W1 / 2, X2 + W2 / 2);
  const double inter = fabs(py_max(yb - ya, 0.0) * py_max(xb - xa, 0.0));
  double iou = 0.0;
  if (!(inter == 0.0)) {
    const double a1 = W1 * H1;
    const double a2 = W2 * H2;
    iou = inter / (a1 + a2 - inter);
  }
  return iou >= thr;
}

// evaluate_keypoints.py:61-71.
__device__ __forceinline__ bool centre_pass(float y1, float x1, float y2, float x2, double thr) {
#pragma clang fp contract(off)
  const double dy = (double)y1 - (double)y2, dx = (double)x1 - (double)x2;
  const double distance = sqrt(dy * dy + dx * dx);
  return !(distance > thr);
}

// A key that orders like the score: larger score, larger key; -0 == +0; NaN below everything.
__device__ __forceinline__ unsigned score_key(float s) {
  if (s != s) return 0u;
  if (s == 0.0f) s = 0.0f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void walk(const Params p) {
  __shared__ unsigned long long s_qual[kMaxK * kWords];  // by rank
  __shared__ unsigned s_key[kMaxK];
  __shared__ float s_score[kMaxK];
  __shared__ int s_det[kMaxK];             // by record
  __shared__ unsigned short s_order[kMaxK];  // rank -> record
  __shared__ long long s_tlab[kMaxN];
  __shared__ float s_ty[kMaxN], s_tx[kMaxN], s_th[kMaxN], s_tw[kMaxN];
  __shared__ unsigned char s_tvalid[kMaxN];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, N = p.N, T = p.T, rs = p.rec_stride;
  const int n = min(max(p.counts[b], 0), K);
  const int nw = (N + 63) >> 6;
  const float* rec = p.records + (size_t)b * K * rs;

  // a. stage
  for (int i = tid; i < n; i += kThreads) {
    const float s = rec[(size_t)i * rs + p.c_score];
    s_score[i] = s;
    s_key[i] = score_key(s);
  }
  for (int m = tid; m < N; m += kThreads) {
    const size_t g = (size_t)b * N + m;
    s_tvalid[m] = p.t_valid[g] != 0;
    s_tlab[m] = p.t_label[g];
    s_ty[m] = p.t_center[g * 2 + 0];
    s_tx[m] = p.t_center[g * 2 + 1];
    s_th[m] = p.t_size ? p.t_size[g * 2 + 0] : 0.0f;
    s_tw[m] = p.t_size ? p.t_size[g * 2 + 1] : 0.0f;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const unsigned ki = s_key[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned kj = s_key[j];
      rank += (kj > ki || (kj == ki && j > i)) ? 1 : 0;
    }
    s_order[rank] = (unsigned short)i;  // the ranks are a permutation of 0 .. n-1
  }
  __syncthreads();

  // b. qualification words: task (rank r, word w) per wave, truth w * 64 + lane per lane
  for (int t = wave; t < n * nw; t += kWaves) {
    const int r = t / nw, w = t - r * nw;
    const int i = s_order[r];
    const float* q = rec + (size_t)i * rs;
    const long long lab = (long long)(int)q[p.c_label];
    const int m = w * 64 + lane;
    bool ok = false;
    if (m < N && s_tvalid[m] && s_tlab[m] == lab) {
      if (p.mode == 0) ok = box_pass(q[p.c_y], q[p.c_x], q[p.c_h], q[p.c_w], s_ty[m], s_tx[m], s_th[m], s_tw[m], p.thr);
      else ok = centre_pass(q[p.c_y], q[p.c_x], s_ty[m], s_tx[m], p.thr);
    }
    const unsigned long long word = __ballot(ok);
    if (lane == 0) s_qual[r * kWords + w] = word;
  }
  __syncthreads();

  // c. the walk
  if (wave == 0) {
    unsigned long long free_mask = ~0ull;  // (a truth that may not be taken has no bit in any qual word)
    for (int r = 0; r < n; ++r) {
      const unsigned long long c = lane < nw ? (s_qual[r * kWords + lane] & free_mask) : 0ull;
      const unsigned long long has = __ballot(c != 0ull);
      int m = -1;
      if (has != 0ull) {
        const int wl = __ffsll((long long)has) - 1;
        const unsigned lo = (unsigned)__shfl((int)(unsigned)c, wl, 64);
        const unsigned hi = (unsigned)__shfl((int)(unsigned)(c >> 32), wl, 64);
        const unsigned long long word = ((unsigned long long)hi << 32) | lo;
        const int bit = __ffsll((long long)word) - 1;
        if (lane == wl) free_mask &= ~(1ull << bit);
        m = wl * 64 + bit;
      }
      if (lane == 0) s_det[s_order[r]] = m;
    }
  }
  __syncthreads();

  // d. outputs and counts
  int* det_truth = p.det_truth + (size_t)b * K;
  for (int i = tid; i < K; i += kThreads) det_truth[i] = i < n ? s_det[i] : -1;
  for (int t = wave; t < T; t += kWaves) {
    const float thr = p.score_thr[t];
    int n_det = 0, n_tp = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool in = i < n && s_score[i] >= thr;
      n_det += __popcll(__ballot(in));
      n_tp += __popcll(__ballot(in && s_det[i] >= 0));
    }
    if (lane == 0) {
      if (n_tp) atomicAdd(p.totals + t, (unsigned long long)n_tp);
      if (n_det) atomicAdd(p.totals + T + t, (unsigned long long)n_det);
    }
  }
  if (wave == kWaves - 1) {
    int n_truth = 0;
    for (int base = 0; base < N; base += 64) {
      const int m = base + lane;
      n_truth += __popcll(__ballot(m < N && s_tvalid[m]));
    }
    if (lane == 0 && n_truth) atomicAdd(p.totals + 2 * T, (unsigned long long)n_truth);
  }
}

}  // namespace evaluate

int launch_evaluate_detections(const float* records, int rec_stride, const int* counts, const int* cols, int B, int K,
                               const uint8_t* truth_valid, const long long* truth_label, const float* truth_center,
                               const float* truth_size, int N, int mode, double match_threshold,
                               const float* score_thresholds, int T, int* det_truth, long long* totals, hipStream_t s) {
  using namespace evaluate;
  if (mode != 0 && mode != 1) { set_error("evaluate_detections: mode must be 0 (box) or 1 (centre)"); return 1; }
  if (!records || !counts || !cols || !truth_valid || !truth_label || !truth_center || (mode == 0 && !truth_size) ||
      !score_thresholds || !det_truth || !totals) {
    set_error("evaluate_detections: null pointer");
    return 1;
  }
  if (B < 0) { set_error("evaluate_detections: negative B"); return 1; }
  if (K < 0 || K > kMaxK) { set_error("evaluate_detections: K must be in 0..1024"); return 1; }
  if (N < 1 || N > kMaxN) { set_error("evaluate_detections: N must be in 1..256"); return 1; }
  if (T < 1 || T > kMaxT) { set_error("evaluate_detections: T must be in 1..64"); return 1; }
  if (rec_stride < 1) { set_error("evaluate_detections: rec_stride must be >= 1"); return 1; }
  for (int i = 0; i < 6; ++i)
    if (cols[i] < 0 || cols[i] >= rec_stride) {
      set_error("evaluate_detections: a column lies outside the record (cols[i] must be in 0..rec_stride-1)");
      return 1;
    }
  if (B == 0 || K == 0) return 0;
  Params p{};
  p.records = records; p.counts = counts; p.rec_stride = rec_stride; p.K = K; p.N = N; p.T = T; p.mode = mode;
  p.c_label = cols[0]; p.c_score = cols[1]; p.c_y = cols[2]; p.c_x = cols[3];
  p.c_h = cols[4]; p.c_w = cols[5];
  p.t_valid = truth_valid; p.t_label = truth_label; p.t_center = truth_center; p.t_size = truth_size;
  p.thr = match_threshold; p.score_thr = score_thresholds; p.det_truth = det_truth;
  p.totals = (unsigned long long*)totals;
  hipLaunchKernelGGL(walk, dim3((unsigned)B), dim3(kThreads), 0, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
