// Object poses from matched keypoints (reference decode.py:137-172, cv2.solvePnP there) for B x K
// detections in one launch, on what tv_decode (mode 1) and tv_match_keypoints leave on the device. The
// contract is tv_solve_poses' in include/tauv_vision_amd.h; the numerics are pose_dev.h's.
//
// One wave (a 64-thread workgroup) per detection, B * K workgroups.
//   1. Lane s < max_slots tests slot s (a model point that is not NaN, a keypoint rank inside the image's
//      count); a ballot compacts the correspondences in slot order into LDS (pose::Work, 3.7 KiB).
//   2. pose::solve: the linear start and the Levenberg-Marquardt polish. The normal matrices and the
//      Jacobi rotations are spread over the lanes; the 3 x 3 and 6 x 6 algebra is computed by every lane in
//      registers from LDS broadcasts, so control flow stays wave-uniform and every loop is bounded.
//   3. Lane 0 stores the 16 columns. Every row of `poses` is written by its own workgroup on every call.
#include "common.h"
#include "pose_dev.h"

#include <cmath>

namespace tv {
namespace pose {

constexpr int kRec = 10;  // columns of a tv_decode record

struct Params {
  const float* obj;        // [B][K][10]
  const int* obj_counts;   // [B]
  const float* kp;         // [B][K_kp][10]
  const int* kp_counts;    // [B]
  const int* slot_kp;      // [B][K][max_slots]
  const float* model;      // [n_labels][max_slots][3]
  int n_labels, max_slots, K, K_kp, in_h, in_w, min_points;
  double fx, fy, cx, cy;
  float* poses;            // [B][K][16]
};

__global__ __launch_bounds__(64) void solve_poses(const Params p) {
  __shared__ Work W;
  const int lane = threadIdx.x;
  const int bd = blockIdx.x, b = bd / p.K, d = bd - b * p.K;
  const int S = p.max_slots;
  const int n_obj = min(max(p.obj_counts[b], 0), p.K);
  const int n_kp = min(max(p.kp_counts[b], 0), p.K_kp);

  bool have = false;
  float X[3] = {0.f, 0.f, 0.f}, ky = 0.f, kx = 0.f;
  if (d < n_obj && lane < S) {
    const float lab = p.obj[(size_t)bd * kRec];
    if (lab > -1.f && lab < (float)p.n_labels) {  // (int)lab in [0, n_labels); false for NaN
      const float* m = p.model + ((size_t)(int)lab * S + lane) * 3;
      X[0] = m[0]; X[1] = m[1]; X[2] = m[2];
      const int k = p.slot_kp[(size_t)bd * S + lane];
      if (X[0] == X[0] && X[1] == X[1] && X[2] == X[2] && k >= 0 && k < n_kp) {
        const float* r = p.kp + ((size_t)b * p.K_kp + k) * kRec;
        ky = r[2];
        kx = r[3];
        have = true;
      }
    }
  }
  const unsigned long long mask = __ballot(have);
  const int n = __popcll(mask);
  if (have) {
    const int i = __popcll(mask & ((1ull << lane) - 1ull));  // lane < 32 here
    W.X[i][0] = (double)X[0]; W.X[i][1] = (double)X[1]; W.X[i][2] = (double)X[2];
    W.u[i] = (double)kx * (double)p.in_w;
    W.v[i] = (double)ky * (double)p.in_h;
  }
  __syncthreads();
  const Result r = solve(W, n, p.fx, p.fy, p.cx, p.cy, p.min_points, Lanes{lane, 64});
  if (lane == 0) store_row(r, n, p.poses + (size_t)bd * kCols);
}

}  // namespace pose

int launch_solve_poses(const float* obj_records, const int* obj_counts, const float* kp_records, const int* kp_counts,
                       const int* slot_kp, const float* model_points, int n_labels, int max_slots, int B, int K,
                       int K_kp, int in_h, int in_w, float fx, float fy, float cx, float cy, int min_points,
                       float* poses, hipStream_t s) {
  using namespace pose;
  if (!obj_records || !obj_counts || !kp_records || !kp_counts || !slot_kp || !model_points || !poses) {
    set_error("solve_poses: null pointer");
    return 1;
  }
  if (B < 0) { set_error("solve_poses: negative B"); return 1; }
  if (K < 1 || K > 256) { set_error("solve_poses: K must be in 1..256"); return 1; }
  if (K_kp < 1 || K_kp > 1024) { set_error("solve_poses: K_kp must be in 1..1024"); return 1; }
  if (max_slots < 1 || max_slots > kMaxPts) { set_error("solve_poses: max_slots must be in 1..32"); return 1; }
  if (n_labels < 1) { set_error("solve_poses: n_labels must be >= 1"); return 1; }
  if (min_points < 6 || min_points > kMaxPts) { set_error("solve_poses: min_points must be in 6..32"); return 1; }
  if (in_h < 1 || in_w < 1) { set_error("solve_poses: in_h and in_w must be positive"); return 1; }
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f) {
    set_error("solve_poses: fx and fy must be finite and non-zero");
    return 1;
  }
  if ((long long)B * K > 0x7fffffffLL / kCols) { set_error("solve_poses: B*K too large"); return 1; }
  if (B == 0) return 0;
  Params p{};
  p.obj = obj_records; p.obj_counts = obj_counts; p.kp = kp_records; p.kp_counts = kp_counts; p.slot_kp = slot_kp;
  p.model = model_points; p.n_labels = n_labels; p.max_slots = max_slots; p.K = K; p.K_kp = K_kp;
  p.in_h = in_h; p.in_w = in_w; p.min_points = min_points;
  p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
  p.poses = poses;
  hipLaunchKernelGGL(solve_poses, dim3((unsigned)(B * K)), dim3(64), 0, s, p);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
