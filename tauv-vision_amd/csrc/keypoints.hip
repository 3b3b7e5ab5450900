// Keypoint-to-object matching of decode_keypoints (reference decode.py:100-135) for B images in one
// launch, on the records tv_decode (mode 1) writes. The reference walks the keypoints of an image in
// score order; each goes to the object of its owner label whose slot is still free and whose
// direction from the keypoint, atan2(ky - y, kx - x), is nearest the keypoint's affinity angle
// atan2(ay, ax) — |difference| in double on the fp32 record values, without wrap-around, first
// index on a tie, first candidate when the affinity is NaN.
//
// One workgroup of 256 threads per image.
//   1. All threads write -1 over the image's slot_kp rows and the kp_det rows past the keypoint
//      count, and stage the objects (label, y, x) and the keypoints (affinity angle, y, x, owner
//      label, owner slot) in LDS.
//   2. Table route (K_kp * K <= kTable entries): all threads fill err[k][d] in LDS, +inf where the
//      label differs — the atan2 of every pair is off the serial chain.
//   3. Wave 0 walks the keypoints in rank order. Lane l owns the objects l, l + 64, l + 128, l + 192
//      (K <= 256): their labels, a taken-slot bitmask (max_slots <= 32) and a match count stay in
//      registers. Per keypoint: each lane's best (error, rank) over its free objects of the owner
//      label, a butterfly argmin over the 64 lanes (skipped when at most one lane has a candidate),
//      and the winning lane sets its bit and stores slot_kp. Without the table (in-walk route) the lane computes the error there, with the same
//      function on the same values: the two routes give identical results.
// An error is never +inf (it is at most 2 pi), so +inf with rank INT_MAX marks "no candidate"; a NaN
// error is carried as +inf with its rank, which makes the first candidate win when all are NaN.
// Every element of the three outputs is written by every call. The only addresses written twice are
// slot_kp's (the -1 fill, then the match, a __syncthreads between them).
#include "common.h"

#include <climits>
#include <cmath>

namespace tv {
namespace keypoints {

constexpr int kThreads = 256;
constexpr int kMaxK = 256;       // 4 objects per lane of the walking wave
constexpr int kMaxKp = 1024;
constexpr int kMaxSlots = 32;    // one bit per slot
constexpr int kTable = 4096;     // error-table entries kept in LDS (32 KiB of doubles)
constexpr int kRec = 10;         // columns of a tv_decode record
constexpr int kPerLane = kMaxK / 64;

struct Params {
  const float* obj;       // [B][K][10]
  const int* obj_counts;  // [B]
  const float* kp;        // [B][K_kp][10]
  const int* kp_counts;   // [B]
  const int* owner_label; // [n_keypoints]
  const int* owner_slot;  // [n_keypoints]
  int n_keypoints, max_slots, K, K_kp;
  int* kp_det;            // [B][K_kp]
  int* slot_kp;           // [B][K][max_slots]
  int* n_matched;         // [B][K]
};

// |ang - atan2(ky - y, kx - x)| as the reference's Python floats form it; NaN -> +inf. Not inlined:
// the table route and the in-walk route run the very same instructions.
__device__ __noinline__ double angle_error(double ang, float ky, float kx, float y, float x) {
#pragma clang fp contract(off)
  const double e = fabs(ang - atan2((double)ky - (double)y, (double)kx - (double)x));
  return e == e ? e : (double)INFINITY;
}

template <bool TABLE>
__global__ __launch_bounds__(kThreads) void match(const Params p) {
  __shared__ double s_tab[TABLE ? kTable : 1];
  __shared__ double s_ang[kMaxKp];
  __shared__ float s_ky[kMaxKp], s_kx[kMaxKp];
  __shared__ short s_owner[kMaxKp], s_slot[kMaxKp];  // -1: the keypoint has no owner (never a candidate)
  __shared__ float s_oy[kMaxK], s_ox[kMaxK];
  __shared__ int s_olab[kMaxK];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = p.K, K_kp = p.K_kp, S = p.max_slots;
  const int n_obj = min(max(p.obj_counts[b], 0), K);
  const int n_kp = min(max(p.kp_counts[b], 0), K_kp);
  const float* obj = p.obj + (size_t)b * K * kRec;
  const float* kp = p.kp + (size_t)b * K_kp * kRec;
  int* kp_det = p.kp_det + (size_t)b * K_kp;
  int* slot_kp = p.slot_kp + (size_t)b * K * S;
  int* n_matched = p.n_matched + (size_t)b * K;

  for (int i = tid; i < K * S; i += kThreads) slot_kp[i] = -1;
  for (int k = n_kp + tid; k < K_kp; k += kThreads) kp_det[k] = -1;
  for (int d = tid; d < n_obj; d += kThreads) {
    s_olab[d] = (int)obj[d * kRec + 0];
    s_oy[d] = obj[d * kRec + 2];
    s_ox[d] = obj[d * kRec + 3];
  }
  for (int k = tid; k < n_kp; k += kThreads) {
    const float* r = kp + k * kRec;
    const int kl = (int)r[0];
    int owner = -1, slot = -1;
    if (kl >= 0 && kl < p.n_keypoints) {
      owner = p.owner_label[kl];
      slot = p.owner_slot[kl];
      if (owner < 0 || owner > SHRT_MAX || slot < 0 || slot >= S) owner = slot = -1;
    }
    s_owner[k] = (short)owner;
    s_slot[k] = (short)slot;
    s_ky[k] = r[2];
    s_kx[k] = r[3];
    s_ang[k] = atan2((double)r[8], (double)r[9]);
  }
  __syncthreads();

  if (TABLE) {
    for (int i = tid; i < n_kp * K; i += kThreads) {
      const int k = i / K, d = i - k * K;
      double e = (double)INFINITY;
      if (d < n_obj && s_olab[d] == (int)s_owner[k]) e = angle_error(s_ang[k], s_ky[k], s_kx[k], s_oy[d], s_ox[d]);
      s_tab[i] = e;
    }
    __syncthreads();
  }
  if (tid >= 64) return;

  const int lane = tid;
  int lab[kPerLane], cnt[kPerLane];
  unsigned taken[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int d = lane + 64 * j;
    lab[j] = d < n_obj ? s_olab[d] : -1;  // -1 never equals an owner label of a keypoint that has one
    cnt[j] = 0;
    taken[j] = 0u;
  }
  const int nj = (n_obj + 63) >> 6;  // wave-uniform: the node's K = 10 walks one object per lane
  for (int k = 0; k < n_kp; ++k) {
    const int owner = s_owner[k], slot = s_slot[k];
    double best_e = (double)INFINITY;
    int best_r = INT_MAX;
    if (owner >= 0) {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        const int d = lane + 64 * j;
        if (j < nj && lab[j] == owner && !((taken[j] >> slot) & 1u)) {
          const double e = TABLE ? s_tab[k * K + d] : angle_error(s_ang[k], s_ky[k], s_kx[k], s_oy[d], s_ox[d]);
          if (e < best_e || best_r == INT_MAX) {  // (d grows with j: an equal error keeps the smaller rank)
            best_e = e;
            best_r = d;
          }
        }
      }
    }
    // Most steps of a sparse scene have no lane, or one lane, with a candidate: then there is nothing to
    // compare and the 6-step butterfly (three cross-lane moves each, all on the serial chain) is skipped.
    const unsigned long long has = __ballot(best_r != INT_MAX);
    if (has != 0 && (has & (has - 1)) == 0) {
      best_r = __shfl(best_r, __ffsll((long long)has) - 1, 64);
    } else if (has != 0) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oe = __shfl_xor(best_e, off, 64);
        const int orank = __shfl_xor(best_r, off, 64);
        if (oe < best_e || (oe == best_e && orank < best_r)) {
          best_e = oe;
          best_r = orank;
        }
      }
    }
    const bool matched = best_r != INT_MAX;
    if (matched && (best_r & 63) == lane) {
      const int jw = best_r >> 6;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j)
        if (j == jw) {
          taken[j] |= 1u << slot;
          cnt[j] += 1;
        }
      slot_kp[best_r * S + slot] = k;
    }
    if (lane == 0) kp_det[k] = matched ? best_r : -1;
  }
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int d = lane + 64 * j;
    if (d < K) n_matched[d] = cnt[j];
  }
}

}  // namespace keypoints

int launch_match_keypoints(const float* obj_records, const int* obj_counts, const float* kp_records,
                           const int* kp_counts, const int* owner_label, const int* owner_slot, int n_keypoints,
                           int max_slots, int B, int K, int K_kp, int* kp_det, int* slot_kp, int* n_matched,
                           hipStream_t s) {
  using namespace keypoints;
  if (!obj_records || !obj_counts || !kp_records || !kp_counts || !owner_label || !owner_slot || !kp_det || !slot_kp ||
      !n_matched) {
    set_error("match_keypoints: null pointer");
    return 1;
  }
  if (B < 0) { set_error("match_keypoints: negative B"); return 1; }
  if (n_keypoints < 1) { set_error("match_keypoints: n_keypoints must be >= 1"); return 1; }
  if (max_slots < 1 || max_slots > kMaxSlots) { set_error("match_keypoints: max_slots must be in 1..32"); return 1; }
  if (K < 1 || K > kMaxK) { set_error("match_keypoints: K must be in 1..256"); return 1; }
  if (K_kp < 1 || K_kp > kMaxKp) { set_error("match_keypoints: K_kp must be in 1..1024"); return 1; }
  if (B == 0) return 0;
  Params p{};
  p.obj = obj_records; p.obj_counts = obj_counts; p.kp = kp_records; p.kp_counts = kp_counts;
  p.owner_label = owner_label; p.owner_slot = owner_slot; p.n_keypoints = n_keypoints; p.max_slots = max_slots;
  p.K = K; p.K_kp = K_kp; p.kp_det = kp_det; p.slot_kp = slot_kp; p.n_matched = n_matched;
  const dim3 grid((unsigned)B), block(kThreads);
  if (K * K_kp <= kTable) hipLaunchKernelGGL(match<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(match<false>, grid, block, 0, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
