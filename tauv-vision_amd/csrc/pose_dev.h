// Numerics of the pose stage (tv_solve_poses, pose.hip): the pose (R, t) of n point correspondences that
// minimises the summed squared pixel reprojection error. __host__ __device__, so the kernel and the host
// check (tools/pose_host_check.cpp) run the same code; the contract is tv_solve_poses' in
// include/tauv_vision_amd.h. Everything is double on the fp32 inputs.
//
//   linear start   The object points are centred and scaled (Hartley). Not coplanar: the 12-parameter DLT
//                  in normalised image coordinates, the null vector of its 12 x 12 normal matrix. Coplanar
//                  (smallest eigenvalue of the centred scatter below 1e-6 of the middle one): the
//                  homography from the plane's own frame, the null vector of a 9 x 9 normal matrix, and its
//                  decomposition [h1 h2 h1 x h2]. The sign makes the mean depth positive; the rotation part
//                  is replaced by the nearest rotation (the two largest singular pairs of M from the
//                  eigenvectors of M^T M, the third axis by cross products, so det = +1 by construction).
//                  No start, and an invalid pose, when all object points or all pixels are equal.
//   polish         Levenberg-Marquardt on the increment (w, dt): R <- exp([w]x) R, t <- t + dt, with the
//                  analytic Jacobian [-Jp [R X]x, Jp], Jp the 2 x 3 Jacobian of the projection. At most
//                  kMaxIter Jacobians, kMaxTries dampings each (lambda in [1e-12, 1e12]); it ends on a step
//                  of at most kStepTol (1 + |t|), or when no damping of the ladder lowers the cost.
//   one Jacobi     jacobi<N> (cyclic, at most kMaxSweeps sweeps) serves the scatter (3), the DLT (12), the
//                  homography (9) and the nearest rotation (3).
//
// Lanes: on the device one wave (a 64-thread workgroup) solves one detection. The matrices live in `Work`
// (LDS there, the stack on the host). The entries of a normal matrix and the rows touched by one Jacobi
// rotation are spread over the lanes (`for (i = L.lane; i < n; i += L.n)`); every scalar that steers
// control flow is computed by every lane from the same LDS values with the same instructions, so control
// flow is wave-uniform and sync() — __syncthreads() of the one-wave workgroup, nothing on the host — is
// reached by all lanes or none. On the host L = {0, 1} and the same loops run serially.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#define TV_HD __host__ __device__ __forceinline__

namespace tv {
namespace pose {

constexpr int kMaxPts = 32;     // max_slots
constexpr int kCols = 16;
constexpr int kMaxSweeps = 30;
constexpr int kMaxIter = 50;
constexpr int kMaxTries = 12;
constexpr double kStepTol = 1e-12;
constexpr double kPlanarRatio = 1e-6;
constexpr double kEps = 2.220446049250313e-16;

struct Lanes { int lane, n; };

struct Work {
  double X[kMaxPts][3];   // object points
  double u[kMaxPts], v[kMaxPts];  // pixels
  double P[kMaxPts][4];   // normalised object points of the linear solve (x, y, z, 1) or (a, b, 1, -)
  double A[144], V[144];  // the symmetric matrix of jacobi<N> and its eigenvectors (columns)
};

struct Result {
  double R[9], t[3], rms;
  int valid, iters;
};

TV_HD void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// Not `x - x == 0`: under fp contraction the compiler may fuse the product that made x into the
// subtraction, which then yields the product's rounding error instead of 0.
TV_HD bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// Cyclic Jacobi on the symmetric N x N matrix A (full storage): on return the diagonal holds the
// eigenvalues and the columns of V the eigenvectors. A rotation is skipped when its off-diagonal element
// is below the rounding of the two diagonal elements (or of the trace: an absolute floor for the null
// space of exact data, or is NaN); a sweep without a rotation ends the routine.
template <int N>
TV_HD void jacobi(double* A, double* V, const Lanes L) {
  for (int i = L.lane; i < N * N; i += L.n) V[i] = (i / N == i % N) ? 1.0 : 0.0;
  sync();
  double tr = 0.0;
  for (int i = 0; i < N; ++i) tr += fabs(A[i * N + i]);
  const double floor_ = 1e-22 * tr;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool any = false;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];
        const double thr = kEps * sqrt(fabs(app * aqq));
        if (!(fabs(apq) > thr) || !(fabs(apq) > floor_)) continue;
        any = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        sync();  // every lane has read the three elements
        for (int k = L.lane; k < N; k += L.n) {
          if (k != p && k != q) {
            const double akp = A[k * N + p], akq = A[k * N + q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            A[k * N + p] = np_; A[p * N + k] = np_;
            A[k * N + q] = nq_; A[q * N + k] = nq_;
          } else if (k == p) {
            A[p * N + p] = app - tt * apq;
            A[q * N + q] = aqq + tt * apq;
            A[p * N + q] = 0.0; A[q * N + p] = 0.0;
          }
          const double vkp = V[k * N + p], vkq = V[k * N + q];
          V[k * N + p] = c * vkp - s * vkq;
          V[k * N + q] = s * vkp + c * vkq;
        }
        sync();
      }
    if (!any) break;
  }
}

TV_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
TV_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
TV_HD void matvec3(const double* M, const double* x, double* y) {  // y = M x, M row-major
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = M[3 * i] * x[0] + M[3 * i + 1] * x[1] + M[3 * i + 2] * x[2];
}
TV_HD void matmul3(const double* A, const double* B, double* C) {  // C = A B
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Eigenvalues w (ascending) and eigenvectors e0, e1, e2 of the symmetric 3 x 3 matrix S (row-major).
TV_HD void eigen3(const double* S, Work& W, const Lanes L, double* w, double* e0, double* e1, double* e2) {
  sync();  // earlier readers of W.A / W.V are done
  if (L.lane == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) W.A[i] = S[i];
  }
  sync();
  jacobi<3>(W.A, W.V, L);
  double d[3], E[3][3];  // E[c]: eigenvector c
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = W.A[4 * c];
#pragma unroll
    for (int k = 0; k < 3; ++k) E[c][k] = W.V[3 * k + c];
  }
  // a three-element sorting network on registers
#define TV_POSE_CSWAP(a, b)                                               \
  if (d[b] < d[a]) {                                                      \
    const double td = d[a]; d[a] = d[b]; d[b] = td;                       \
    _Pragma("unroll") for (int k = 0; k < 3; ++k) {                       \
      const double te = E[a][k]; E[a][k] = E[b][k]; E[b][k] = te;         \
    }                                                                     \
  }
  TV_POSE_CSWAP(0, 1)
  TV_POSE_CSWAP(1, 2)
  TV_POSE_CSWAP(0, 1)
#undef TV_POSE_CSWAP
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = d[k];
    e0[k] = E[0][k]; e1[k] = E[1][k]; e2[k] = E[2][k];
  }
}

// The rotation nearest M (row-major) and the matching scale; false when M has no two directions.
TV_HD bool nearest_rotation(const double* M, Work& W, const Lanes L, double* R, double* scale) {
  double S[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[3 * i + j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
  double w[3], v3[3], v2[3], v1[3];
  eigen3(S, W, L, w, v3, v2, v1);  // ascending: v1 belongs to the largest
  if (!(w[1] > 0.0) || !finite(w[2])) return false;
  const double s1 = sqrt(w[2]), s2 = sqrt(w[1]);
  double u1[3], u2[3], u3[3], t3[3];
  matvec3(M, v1, u1);
  matvec3(M, v2, u2);
#pragma unroll
  for (int k = 0; k < 3; ++k) { u1[k] /= s1; u2[k] /= s2; }
  const double n1 = sqrt(dot3(u1, u1));
#pragma unroll
  for (int k = 0; k < 3; ++k) u1[k] /= n1;
  const double d12 = dot3(u1, u2);  // 0 already unless the second singular value is at rounding level
#pragma unroll
  for (int k = 0; k < 3; ++k) u2[k] -= d12 * u1[k];
  const double n2 = sqrt(dot3(u2, u2));
#pragma unroll
  for (int k = 0; k < 3; ++k) u2[k] /= n2;
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
  matvec3(M, v3, t3);
  *scale = (s1 + s2 + dot3(u3, t3)) / 3.0;
  return true;
}

// Element j of design row r (0: the x equation, 1: the y equation) of a point with homogeneous
// coordinates Ph[0..D): [Ph 0 -x Ph] and [0 Ph -y Ph].
template <int D>
TV_HD double design(const double* Ph, double x, double y, int r, int j) {
  const int blk = j / D, c = j - blk * D;
  const double p = Ph[c];
  return blk == 2 ? -(r ? y : x) * p : (blk == r ? p : 0.0);
}

// The null vector (unit eigenvector of the smallest eigenvalue) of the 3D x 3D normal matrix of the n
// design rows over W.P and the normalised image points (fx, fy, cx, cy take the pixels there).
template <int D>
TV_HD void null_vector(Work& W, int n, double fx, double fy, double cx, double cy, const Lanes L, double* p) {
  constexpr int N = 3 * D;
  sync();
  for (int e = L.lane; e < N * N; e += L.n) {
    const int i = e / N, j = e - i * N;
    double acc = 0.0;
    for (int k = 0; k < n; ++k) {
      const double x = (W.u[k] - cx) / fx, y = (W.v[k] - cy) / fy;
      acc += design<D>(W.P[k], x, y, 0, i) * design<D>(W.P[k], x, y, 0, j) +
             design<D>(W.P[k], x, y, 1, i) * design<D>(W.P[k], x, y, 1, j);
    }
    W.A[e] = acc;
  }
  sync();
  jacobi<N>(W.A, W.V, L);
  int best = 0;
  double lo = W.A[0];
  for (int i = 1; i < N; ++i) {
    const double d = W.A[i * N + i];
    if (d < lo) { lo = d; best = i; }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) p[k] = W.V[k * N + best];
}

// The linear start. false: the points have no extent, or the solve broke down.
TV_HD bool initial_pose(Work& W, int n, double fx, double fy, double cx, double cy, const Lanes L, double* R, double* t) {
  double m[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < n; ++k) { m[0] += W.X[k][0]; m[1] += W.X[k][1]; m[2] += W.X[k][2]; }
  m[0] /= n; m[1] /= n; m[2] /= n;
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; ++k) {
    const double d[3] = {W.X[k][0] - m[0], W.X[k][1] - m[1], W.X[k][2] - m[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[3 * i + j] += d[i] * d[j];
  }
  double w[3], e0[3], e1[3], e2[3];
  eigen3(S, W, L, w, e0, e1, e2);
  if (!finite(w[0]) || !finite(w[1]) || !finite(w[2]) || !(w[2] > 0.0)) return false;
  sync();
  if (w[0] < kPlanarRatio * w[1]) {
    // coplanar: (a, b) in the plane's frame [e2 e1 e2 x e1], a homography, its decomposition
    double en[3];
    cross3(e2, e1, en);
    const double sc = sqrt(2.0 * n / (w[1] + w[2]));
    for (int k = L.lane; k < n; k += L.n) {
      const double d[3] = {W.X[k][0] - m[0], W.X[k][1] - m[1], W.X[k][2] - m[2]};
      W.P[k][0] = sc * dot3(d, e2);
      W.P[k][1] = sc * dot3(d, e1);
      W.P[k][2] = 1.0;
      W.P[k][3] = 0.0;
    }
    double h[9];
    null_vector<3>(W, n, fx, fy, cx, cy, L, h);
    double depth = 0.0;
    for (int k = 0; k < n; ++k) depth += h[6] * W.P[k][0] + h[7] * W.P[k][1] + h[8];
    const double sg = depth < 0.0 ? -1.0 : 1.0;
    const double h1[3] = {sg * h[0], sg * h[3], sg * h[6]}, h2[3] = {sg * h[1], sg * h[4], sg * h[7]};
    const double lam = 0.5 * (sqrt(dot3(h1, h1)) + sqrt(dot3(h2, h2)));
    if (!(lam > 0.0)) return false;
    double h3[3], M[9], Rh[9], scale;
    cross3(h1, h2, h3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      M[3 * i] = h1[i] / lam;
      M[3 * i + 1] = h2[i] / lam;
      M[3 * i + 2] = h3[i] / (lam * lam);
    }
    if (!nearest_rotation(M, W, L, Rh, &scale)) return false;
    // R = Rh Rp^T, Rp = [e2 e1 en] as columns
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[3 * i + j] = Rh[3 * i] * e2[j] + Rh[3 * i + 1] * e1[j] + Rh[3 * i + 2] * en[j];
    double Rm[3];
    matvec3(R, m, Rm);
    t[0] = sg * h[2] / (lam * sc) - Rm[0];
    t[1] = sg * h[5] / (lam * sc) - Rm[1];
    t[2] = sg * h[8] / (lam * sc) - Rm[2];
    return true;
  }
  const double sc = sqrt(3.0 * n / (w[0] + w[1] + w[2]));
  for (int k = L.lane; k < n; k += L.n) {
    W.P[k][0] = sc * (W.X[k][0] - m[0]);
    W.P[k][1] = sc * (W.X[k][1] - m[1]);
    W.P[k][2] = sc * (W.X[k][2] - m[2]);
    W.P[k][3] = 1.0;
  }
  double p[12];
  null_vector<4>(W, n, fx, fy, cx, cy, L, p);
  double depth = 0.0;
  for (int k = 0; k < n; ++k) depth += p[8] * W.P[k][0] + p[9] * W.P[k][1] + p[10] * W.P[k][2] + p[11];
  const double sg = depth < 0.0 ? -1.0 : 1.0;
  double M[9], scale;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = sg * p[4 * i + j];
  if (!nearest_rotation(M, W, L, R, &scale) || !(scale > 0.0)) return false;
  double Rm[3];
  matvec3(R, m, Rm);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = sg * p[4 * i + 3] / (scale * sc) - Rm[i];
  return true;
}

// R2 = exp([w]x) R (Rodrigues).
TV_HD void rotate_left(const double* w, const double* R, double* R2) {
  const double th2 = dot3(w, w), th = sqrt(th2);
  double a = 1.0, b = 0.5;
  if (th >= 1e-8) {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      E[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K[3 * i + j] + b * (w[i] * w[j] - (i == j ? th2 : 0.0));
  matmul3(E, R, R2);
}

// The summed squared pixel error at (R, t); *front: every point has positive depth.
TV_HD double cost_of(const Work& W, int n, double fx, double fy, double cx, double cy, const double* R,
                     const double* t, bool* front) {
  double cost = 0.0;
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    double Y[3];
    matvec3(R, W.X[k], Y);
    const double x = Y[0] + t[0], y = Y[1] + t[1], z = Y[2] + t[2];
    const double ru = fx * x / z + cx - W.u[k], rv = fy * y / z + cy - W.v[k];
    cost += ru * ru + rv * rv;
    ok = ok && z > 0.0;
  }
  *front = ok;
  return cost;
}

// d = -(H + lam diag H)^-1 g by Cholesky (H symmetric 6 x 6, upper part read); false when not positive definite.
TV_HD bool damped_step(const double (&H)[6][6], const double (&g)[6], double lam, double (&d)[6]) {
#pragma clang fp contract(off)  // the host and the device run the same operation sequence
  double Lm[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j] * (1.0 + lam);
#pragma unroll
    for (int k = 0; k < j; ++k) s -= Lm[j][k] * Lm[j][k];
    ok = ok && s > 0.0 && finite(s);
    const double ljj = sqrt(s);
    Lm[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = H[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) a -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = a / ljj;
    }
  }
  if (!ok) return false;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) a -= Lm[i][k] * y[k];
    y[i] = a / Lm[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double a = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) a -= Lm[k][i] * d[k];
    d[i] = a / Lm[i][i];
  }
  return true;
}

// Levenberg-Marquardt from (R, t), in place. Returns converged; *cost, *iters.
TV_HD bool refine(const Work& W, int n, double fx, double fy, double cx, double cy, double* R, double* t,
                  double* cost_out, int* iters_out) {
#pragma clang fp contract(off)  // as damped_step
  bool front;
  double cost = cost_of(W, n, fx, fy, cx, cy, R, t, &front);
  *cost_out = cost;
  *iters_out = 0;
  if (!finite(cost)) return false;
  double lam = 1e-3;
  int iters = 0;
  bool converged = false;
  while (iters < kMaxIter && !converged) {
    double H[6][6], g[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      g[i] = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) H[i][j] = 0.0;
    }
    for (int k = 0; k < n; ++k) {
      double Y[3];
      matvec3(R, W.X[k], Y);
      const double x = Y[0] + t[0], y = Y[1] + t[1], z = Y[2] + t[2], iz = 1.0 / z;
      const double ru = fx * x * iz + cx - W.u[k], rv = fy * y * iz + cy - W.v[k];
      const double a = fx * iz, c = -fx * x * iz * iz, b = fy * iz, dd = -fy * y * iz * iz;
      const double J0[6] = {c * Y[1], a * Y[2] - c * Y[0], -a * Y[1], a, 0.0, c};
      const double J1[6] = {dd * Y[1] - b * Y[2], -dd * Y[0], b * Y[0], 0.0, b, dd};
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        g[i] += J0[i] * ru + J1[i] * rv;
#pragma unroll
        for (int j = i; j < 6; ++j) H[i][j] += J0[i] * J0[j] + J1[i] * J1[j];
      }
    }
    ++iters;
    bool moved = false;
    for (int tries = 0; tries < kMaxTries && !moved && !converged; ++tries) {
      double d[6];
      if (!damped_step(H, g, lam, d)) {
        lam = fmin(lam * 10.0, 1e12);
        continue;
      }
      double R2[9];
      rotate_left(d, R, R2);
      const double t2[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
      const double c2 = cost_of(W, n, fx, fy, cx, cy, R2, t2, &front);
      double dn = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) dn += d[i] * d[i];
      const bool small = sqrt(dn) <= kStepTol * (1.0 + sqrt(dot3(t, t)));
      if (finite(c2) && c2 <= cost) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = R2[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = t2[i];
        cost = c2;
        moved = true;
        lam = fmax(lam * 0.1, 1e-12);
      }
      if (small) converged = true;
      else if (!moved) lam = fmin(lam * 10.0, 1e12);
    }
    if (!moved) converged = true;  // no damping of the ladder lowers the cost: a minimum to rounding
  }
  *cost_out = cost;
  *iters_out = iters;
  return converged;
}

// One detection: the n points of W.X / W.u / W.v. Every lane returns the same Result.
TV_HD Result solve(Work& W, int n, double fx, double fy, double cx, double cy, int min_points, const Lanes L) {
  Result r;
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 9; ++i) r.R[i] = nan;
  r.t[0] = r.t[1] = r.t[2] = r.rms = nan;
  r.valid = 0;
  r.iters = 0;
  if (n < min_points || n > kMaxPts) return r;
  bool ok = true;
  for (int k = 0; k < n; ++k)
    ok = ok && finite(W.X[k][0]) && finite(W.X[k][1]) && finite(W.X[k][2]) && finite((W.u[k] - cx) / fx) &&
         finite((W.v[k] - cy) / fy);
  if (!ok) return r;
  bool model_extent = false, picture_extent = false;  // not all object points equal, not all pixels equal
  for (int k = 1; k < n; ++k) {
    model_extent = model_extent || W.X[k][0] != W.X[0][0] || W.X[k][1] != W.X[0][1] || W.X[k][2] != W.X[0][2];
    picture_extent = picture_extent || W.u[k] != W.u[0] || W.v[k] != W.v[0];
  }
  if (!model_extent || !picture_extent) return r;
  double R[9], t[3];
  if (!initial_pose(W, n, fx, fy, cx, cy, L, R, t)) return r;
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && finite(R[i]);
  ok = ok && finite(t[0]) && finite(t[1]) && finite(t[2]);
  if (!ok) return r;
  double cost;
  const bool converged = refine(W, n, fx, fy, cx, cy, R, t, &cost, &r.iters);
  bool front;
  const double c2 = cost_of(W, n, fx, fy, cx, cy, R, t, &front);
  ok = converged && front && finite(c2) && finite(cost);
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && finite(R[i]);
  ok = ok && finite(t[0]) && finite(t[1]) && finite(t[2]);
  if (!ok) return r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.R[i] = R[i];
  r.t[0] = t[0]; r.t[1] = t[1]; r.t[2] = t[2];
  r.rms = sqrt(cost / n);
  r.valid = 1;
  return r;
}

// The 16 output columns of a Result with n points.
TV_HD void store_row(const Result& r, int n, float* out) {
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = (float)r.R[i];
  out[9] = (float)r.t[0]; out[10] = (float)r.t[1]; out[11] = (float)r.t[2];
  out[12] = (float)r.valid;
  out[13] = (float)n;
  out[14] = (float)r.rms;
  out[15] = (float)r.iters;
}

}  // namespace pose
}  // namespace tv
