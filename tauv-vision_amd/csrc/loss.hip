// The CenterNet training loss with its gradients (reference loss.py:178-390), gfx950. The contract is
// tv_centernet_loss_* in include/tauv_vision_amd.h.
//
// The reference materialises every target plane, makes four elementwise passes per focal term, gathers
// each head of each object with one indexing op and one host round trip, and autograd builds the same
// number of launches again on the way back. Here:
//   dense     one thread owns V consecutive cells (V = 4 on the vector route, else 1) of one plane of
//             one sample. The cell's target comes from targets_dev.h (the functions tv_train_heatmap /
//             tv_train_keypoint_targets run), so no plane is stored; the logit is read once and the
//             unscaled gradient written once, in the tensor's dtype, through the tensor's own strides.
//             A workgroup's three sums and its positive count are reduced by wave shuffles, then over
//             its four waves in LDS, and stored with plain stores. The extra plane index L + K
//             zero-fills the object heads' gradients for the object kernel.
//   objects   one thread per sample walks the sample's objects in order (two objects can share a cell:
//             the cell's first object sums their gradients in fp32, in object order, and stores once).
//   finalize  one workgroup sums the partial sums in a fixed order (in double), applies focal_loss's
//             N == 0 branch, n_valid = min(count, 1) and the lambdas, and forms the total by the
//             reference's sequence of fp32 additions.
// No float atomics, no waiting between workgroups: a call's bits depend on its inputs alone.
#include "conv_common.h"
#include "targets_dev.h"

#include "../../include/tauv_vision_amd.h"

namespace tv {
namespace loss {

constexpr int kThreads = 256;
constexpr int kDenseF = 4;    // floats a dense workgroup stores: positive, negative, squared error, count
constexpr int kObjF = 16;     // floats a sample stores (Obj* below)
enum { ObjSize = 0, ObjOffset, ObjRoll, ObjPitch, ObjYaw, ObjDepth, ObjValid, ObjErrSum, ObjErrCount, ObjErrMax };

struct View {  // a tensor and its gradient (element strides)
  const void* p;
  void* g;
  long long st[5], gst[5];
};

struct Params {
  targets::Truth t;
  View v[TV_LOSS_TENSORS];
  const float *size, *roll, *pitch, *yaw, *depth;  // truth [B][n_obj]([2])
  const float* angle_range;                        // [3][L]
  int B, L, K, gx;
  float den_heat, den_kp, den_aff, alpha, beta;
  float bin_center[2], bin_min[2], bin_max[2];
  int bin_wraps[2];                                // range_min >= range_max: the bin crosses 0
  float l_kh, l_aff, l_size, l_offset, l_angle, l_depth;
  float* dense_part;  // [B][L + K][gx][kDenseF]
  float* obj_part;    // [B][kObjF]
};

// torch.pow(x, e) for a Python float e: x*x and x*x*x as torch's kernel takes them, (x*x)*(x*x) for the
// usual beta = 4 (within an ulp of std::pow, without its cost on every negative cell), else powf
__device__ __forceinline__ float pw(float x, float e) {
  return e == 2.f ? x * x : e == 1.f ? x : e == 3.f ? x * x * x : e == 4.f ? (x * x) * (x * x) : powf(x, e);
}
__device__ __forceinline__ float sigmoid(float z) { return __fdiv_rn(1.f, 1.f + expf(-z)); }
__device__ __forceinline__ float sign(float d) { return d != d ? d : (float)((d > 0.f) - (d < 0.f)); }

// One cell of focal_loss (loss.py:302-317) on the logit z with target t: adds loss_p / loss_n to
// the sums and returns d(-(loss_p + loss_n)) / dz. isclose(t, 1): |t - 1| <= atol + rtol * 1.
__device__ __forceinline__ float focal_cell(float z, float t, float alpha, float beta, float& pos, float& neg,
                                            float& cnt) {
  const float p = sigmoid(z), q = 1.f - p;
  float dldp;
  if (fabsf(t - 1.f) <= 1e-8f + 1e-5f) {
    const float lg = logf(fmaxf(p, 1e-4f));
    pos += pw(q, alpha) * lg;
    cnt += 1.f;
    dldp = -alpha * pw(q, alpha - 1.f) * lg + (p >= 1e-4f ? __fdiv_rn(pw(q, alpha), p) : 0.f);
  } else {
    const float w = pw(1.f - t, beta), lg = logf(fmaxf(q, 1e-4f));
    neg += w * pw(p, alpha) * lg;
    dldp = w * (alpha * pw(p, alpha - 1.f) * lg - (q >= 1e-4f ? __fdiv_rn(pw(p, alpha), q) : 0.f));
  }
  return -dldp * (q * p);  // sigmoid's backward: grad * (1 - p) * p
}

template <typename T, int V> struct alignas(sizeof(T) * V) Vec { T e[V]; };

template <typename T, int V>
__device__ __forceinline__ void load(const void* base, long long off, float (&z)[V]) {
  const T* p = reinterpret_cast<const T*>(base) + off;
  if (V > 1) {
    const Vec<T, V> v = *reinterpret_cast<const Vec<T, V>*>(p);  // aligned: checked by the launcher
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = to_f<T>(v.e[j]);
  } else {
    z[0] = to_f<T>(p[0]);
  }
}
template <typename T, int V>
__device__ __forceinline__ void store(void* base, long long off, const float (&g)[V]) {
  T* p = reinterpret_cast<T*>(base) + off;
  if (V > 1) {
    Vec<T, V> v;
#pragma unroll
    for (int j = 0; j < V; ++j) v.e[j] = from_f<T>(g[j]);
    *reinterpret_cast<Vec<T, V>*>(p) = v;
  } else {
    p[0] = from_f<T>(g[0]);
  }
}

// sum over the workgroup in a fixed order: 64-lane butterfly, then the four waves in wave order
__device__ __forceinline__ float block_sum(float v, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid (gx, L + K + 1, B). On the vector route (V = 4) H * W is a multiple of 4 and a row of cells is
// contiguous, so a thread's cells q .. q + 3 are one aligned vector of its plane.
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void dense(const Params p) {
  __shared__ float lds[4];
  const int H = p.t.H, W = p.t.W, HW = H * W;
  const int plane = blockIdx.y, b = blockIdx.z;
  const int q0 = (blockIdx.x * kThreads + threadIdx.x) * V;
  const bool live = q0 < HW;
  const int y0 = live ? q0 / W : 0, x0 = live ? q0 - y0 * W : 0;

  if (plane == p.L + p.K) {  // zero the object heads' gradients at this thread's cells
    if (!live) return;
    for (int i = TV_LOSS_SIZE; i < TV_LOSS_TENSORS; ++i) {
      const View& v = p.v[i];
      if (!v.g) continue;
      const int C = i == TV_LOSS_DEPTH ? 1 : i <= TV_LOSS_OFFSET ? 2 : 4;
      for (int j = 0; j < V; ++j) {
        const int q = q0 + j, y = q / W, x = q - y * W;
        T* g = reinterpret_cast<T*>(v.g) + b * v.gst[0] + y * v.gst[1] + x * v.gst[2];
        for (int c = 0; c < C; ++c) g[c * v.gst[3]] = from_f<T>(0.f);
      }
    }
    return;
  }

  float pos = 0.f, neg = 0.f, mse = 0.f, cnt = 0.f;
  if (live && plane < p.L) {
    const View& v = p.v[TV_LOSS_HEATMAP];
    float z[V], g[V];
    load<T, V>(v.p, b * v.st[0] + plane * v.st[1] + y0 * v.st[2] + x0 * v.st[3], z);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = q0 + j, y = V > 1 ? q / W : y0, x = V > 1 ? q - y * W : x0;
      g[j] = focal_cell(z[j], targets::heat_cell(p.t, b, plane, y, x, p.den_heat), p.alpha, p.beta, pos, neg, cnt);
    }
    if (v.g) store<T, V>(v.g, b * v.gst[0] + plane * v.gst[1] + y0 * v.gst[2] + x0 * v.gst[3], g);
  } else if (live) {
    const int k = plane - p.L;
    const View& vh = p.v[TV_LOSS_KEYPOINT_HEATMAP];
    const View& va = p.v[TV_LOSS_KEYPOINT_AFFINITY];
    float z[V], g[V], a0[V], a1[V], g0[V], g1[V];
    load<T, V>(vh.p, b * vh.st[0] + k * vh.st[1] + y0 * vh.st[2] + x0 * vh.st[3], z);
    if (va.p) {
      const long long off = b * va.st[0] + k * va.st[1] + y0 * va.st[3] + x0 * va.st[4];
      load<T, V>(va.p, off, a0);
      load<T, V>(va.p, off + va.st[2], a1);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = q0 + j, y = V > 1 ? q / W : y0, x = V > 1 ? q - y * W : x0;
      const targets::KeypointCell c = targets::keypoint_cell(p.t, b, k, y, x, p.den_kp, p.den_aff);
      g[j] = focal_cell(z[j], c.heat, p.alpha, p.beta, pos, neg, cnt);
      if (va.p) {  // F.mse_loss(reduction="none") * weight (loss.py:245-246); backward 2 (pred - target)
        const float d0 = a0[j] - c.a0, d1 = a1[j] - c.a1;
        mse += c.weight * (d0 * d0);
        mse += c.weight * (d1 * d1);
        g0[j] = c.weight * (2.f * d0);
        g1[j] = c.weight * (2.f * d1);
      }
    }
    if (vh.g) store<T, V>(vh.g, b * vh.gst[0] + k * vh.gst[1] + y0 * vh.gst[2] + x0 * vh.gst[3], g);
    if (va.p && va.g) {
      const long long off = b * va.gst[0] + k * va.gst[1] + y0 * va.gst[3] + x0 * va.gst[4];
      store<T, V>(va.g, off, g0);
      store<T, V>(va.g, off + va.gst[2], g1);
    }
  }
  pos = block_sum(pos, lds);
  neg = block_sum(neg, lds);
  mse = block_sum(mse, lds);
  cnt = block_sum(cnt, lds);
  if (threadIdx.x == 0) {
    float* o = p.dense_part + (((size_t)b * (p.L + p.K) + plane) * p.gx + blockIdx.x) * kDenseF;
    o[0] = pos; o[1] = neg; o[2] = mse; o[3] = cnt;
  }
}

// element (b, y, x, c) of an object head
template <typename T>
__device__ __forceinline__ float head(const View& v, int b, int y, int x, int c) {
  return to_f<T>(reinterpret_cast<const T*>(v.p)[b * v.st[0] + y * v.st[1] + x * v.st[2] + c * v.st[3]]);
}

// the gradients of one cell's object heads, summed in fp32 over the objects that share the cell
struct CellGrad {
  float g[TV_LOSS_TENSORS][4];
};

// torch.remainder(a, r) on fp32 (fmod, moved to the divisor's sign)
__device__ __forceinline__ float remainder(float a, float r) {
  float m = fmodf(a, r);
  if (m != 0.f && ((r < 0.f) != (m < 0.f))) m += r;
  return m;
}

// angle_loss (loss.py:334-376) of one object; adds f * d(result) to the bin / offset gradients gb / go
template <typename T>
__device__ float angle_object(const Params& p, const View& vb, const View& vo, float* gb, float* go, int b, int y,
                              int x, float truth, float range, float f) {
  const float two_pi = (float)6.283185307179586;
  float t = remainder(truth, range);
  t = t * (__fdiv_rn(1.f, range) * two_pi);  // truth * (2 * pi / theta_range): reciprocal, then the scalar
  const float ta = remainder(t, two_pi);     // angle_in_range's angles % (2 * pi)
  float result = 0.f, off_sum = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const bool lo = p.bin_min[i] <= ta, hi = ta <= p.bin_max[i];
    const int inside = p.bin_wraps[i] ? (lo || hi) : (lo && hi);
    // F.cross_entropy over [outside, inside]
    const float l0 = head<T>(vb, b, y, x, 2 * i), l1 = head<T>(vb, b, y, x, 2 * i + 1);
    const float m = fmaxf(l0, l1);
    const float lse = m + logf(expf(l0 - m) + expf(l1 - m));
    result += lse - (inside ? l1 : l0);
    gb[2 * i] += f * (expf(l0 - lse) - (inside ? 0.f : 1.f));
    gb[2 * i + 1] += f * (expf(l1 - lse) - (inside ? 1.f : 0.f));
    // inside * (|offset - sin| + |offset - cos|)
    const float d = t - p.bin_center[i];
    const float ds = head<T>(vo, b, y, x, 2 * i) - sinf(d), dc = head<T>(vo, b, y, x, 2 * i + 1) - cosf(d);
    off_sum += (float)inside * (fabsf(ds) + fabsf(dc));
    go[2 * i] += f * ((float)inside * sign(ds));
    go[2 * i + 1] += f * ((float)inside * sign(dc));
  }
  return result + off_sum;
}

// out_index_for_position (loss.py:138-142) of object bo and its pixel offset (:263-264): both truncate
struct ObjCell {
  int y, x;
  float off[2];
};
__device__ __forceinline__ ObjCell obj_cell(const targets::Truth& t, size_t bo) {
  const float py = __fmul_rn(t.center[2 * bo], (float)t.in_h), px = __fmul_rn(t.center[2 * bo + 1], (float)t.in_w);
  const long long iy = (long long)__fdiv_rn(py, (float)t.ratio), ix = (long long)__fdiv_rn(px, (float)t.ratio);
  ObjCell c;
  c.y = (int)min(max(iy, 0ll), (long long)t.H - 1);
  c.x = (int)min(max(ix, 0ll), (long long)t.W - 1);
  c.off[0] = py - (float)(t.ratio * iy);
  c.off[1] = px - (float)(t.ratio * ix);
  return c;
}

// One thread per sample. The first object of a cell sums the gradients of every object of that cell in
// fp32, in object order, and stores them once over the dense kernel's zeros: no read-modify-write, and a
// half gradient is rounded once however many objects share the cell.
template <typename T>
__global__ __launch_bounds__(64) void objects(const Params p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  const int n = p.t.n_obj;
  int count = 0;  // truth.valid.sum() over the whole batch
  for (int i = 0; i < p.B * n; ++i) count += p.t.valid[i] ? 1 : 0;
  const float n_valid = (float)min(count, 1);  // loss.py:231
  const float f_size = __fdiv_rn(p.l_size, n_valid), f_offset = __fdiv_rn(p.l_offset, n_valid);
  const float f_angle = (float)count * __fdiv_rn(p.l_angle, n_valid), f_depth = __fdiv_rn(p.l_depth, n_valid);
  const float* truth[3] = {p.roll, p.pitch, p.yaw};
  float s[kObjF] = {};
  for (int first = 0; first < n; ++first) {
    const ObjCell c0 = obj_cell(p.t, (size_t)b * n + first);
    bool seen = false;
    for (int o = 0; o < first; ++o) {
      const ObjCell c = obj_cell(p.t, (size_t)b * n + o);
      seen = seen || (c.y == c0.y && c.x == c0.x);
    }
    if (seen) continue;
    const int y = c0.y, x = c0.x;
    CellGrad cg = {};
    for (int o = first; o < n; ++o) {
      const size_t bo = (size_t)b * n + o;
      const ObjCell c = obj_cell(p.t, bo);
      if (c.y != y || c.x != x) continue;
      const float valid = p.t.valid[bo] ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float d = head<T>(p.v[TV_LOSS_SIZE], b, y, x, k) - p.size[2 * bo + k];
        s[ObjSize] += valid * fabsf(d);
        cg.g[TV_LOSS_SIZE][k] += f_size * (valid * sign(d));
        if (valid != 0.f && d == d) {  // nanmean / max over the valid objects' finite errors (:256-258)
          s[ObjErrSum] += fabsf(d);
          s[ObjErrCount] += 1.f;
          s[ObjErrMax] = fmaxf(s[ObjErrMax], fabsf(d));
        }
        const float e = head<T>(p.v[TV_LOSS_OFFSET], b, y, x, k) - c.off[k];
        s[ObjOffset] += valid * fabsf(e);
        cg.g[TV_LOSS_OFFSET][k] += f_offset * (valid * sign(e));
      }
      const long long lab = p.t.label[bo];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const View& vb = p.v[TV_LOSS_ROLL_BIN + 2 * a];
        if (!vb.p) continue;
        const float range = lab >= 0 && lab < p.L ? p.angle_range[(size_t)a * p.L + lab] : 0.f;
        s[ObjRoll + a] += angle_object<T>(p, vb, p.v[TV_LOSS_ROLL_OFFSET + 2 * a], cg.g[TV_LOSS_ROLL_BIN + 2 * a],
                                          cg.g[TV_LOSS_ROLL_OFFSET + 2 * a], b, y, x, truth[a][bo], range, f_angle);
      }
      const View& vd = p.v[TV_LOSS_DEPTH];
      if (vd.p) {  // |1 / sigmoid(d) - 1 - truth| (loss.py:379-390)
        const float sg = sigmoid(head<T>(vd, b, y, x, 0)), r = __fdiv_rn(1.f, sg);
        const float d = (r - 1.f) - p.depth[bo];
        s[ObjDepth] += valid * fabsf(d);
        cg.g[TV_LOSS_DEPTH][0] += (f_depth * (valid * sign(d))) * (-(r * r)) * ((1.f - sg) * sg);
      }
      s[ObjValid] += valid;
    }
#pragma unroll
    for (int i = TV_LOSS_SIZE; i < TV_LOSS_TENSORS; ++i) {
      const View& v = p.v[i];
      if (!v.p || !v.g) continue;
      const int C = i == TV_LOSS_DEPTH ? 1 : i <= TV_LOSS_OFFSET ? 2 : 4;
      T* g = reinterpret_cast<T*>(v.g) + b * v.gst[0] + y * v.gst[1] + x * v.gst[2];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < C) g[k * v.gst[3]] = from_f<T>(cg.g[i][k]);
    }
  }
  for (int i = 0; i < kObjF; ++i) p.obj_part[(size_t)b * kObjF + i] = s[i];
}

// sum over the workgroup in double: a fixed tree
__device__ double block_sum_d(double v, double* lds) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(kThreads) void finalize(const Params p, float* __restrict__ out) {
  __shared__ double lds[kThreads];
  const int P = p.L + p.K, nb = p.B * P * p.gx, tid = threadIdx.x;
  double d[7] = {};  // heatmap: positive, negative, count; keypoints: positive, negative, count, squared error
  for (int i = tid; i < nb; i += kThreads) {
    const float* v = p.dense_part + (size_t)i * kDenseF;
    const int o = (i / p.gx) % P < p.L ? 0 : 3;
    d[o] += v[0]; d[o + 1] += v[1]; d[o + 2] += v[3];
    if (o) d[6] += v[2];
  }
  double s[kObjF] = {};
  float err_max = 0.f;
  for (int b = tid; b < p.B; b += kThreads) {
    for (int i = 0; i < kObjF; ++i) s[i] += p.obj_part[(size_t)b * kObjF + i];
    err_max = fmaxf(err_max, p.obj_part[(size_t)b * kObjF + ObjErrMax]);
  }
  for (int i = 0; i < 7; ++i) d[i] = block_sum_d(d[i], lds);
  for (int i = 0; i < ObjErrMax; ++i) s[i] = block_sum_d(s[i], lds);
  __syncthreads();
  lds[tid] = err_max;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < kThreads; ++i) err_max = fmaxf(err_max, (float)lds[i]);

  const View* v = p.v;
  const float count = (float)s[ObjValid], n_valid = fminf(count, 1.f);
  // focal_loss: -(loss_p + loss_n) / N, or -loss_p when N == 0
  const float n_h = (float)d[2], n_k = (float)d[5];
  const float heat = n_h == 0.f ? -(float)d[0] : __fdiv_rn(-(float)(d[0] + d[1]), n_h);
  float total = heat;
  for (int i = 0; i < 32; ++i) out[i] = 0.f;
  out[11] = heat; out[12] = n_h; out[13] = n_k; out[14] = count;
  out[16 + TV_LOSS_HEATMAP] = n_h == 0.f ? 0.f : __fdiv_rn(1.f, n_h);
  if (v[TV_LOSS_KEYPOINT_HEATMAP].p) {
    const float kh = p.l_kh * (n_k == 0.f ? -(float)d[3] : __fdiv_rn(-(float)(d[3] + d[4]), n_k));
    out[1] = kh;
    out[16 + TV_LOSS_KEYPOINT_HEATMAP] = n_k == 0.f ? 0.f : __fdiv_rn(p.l_kh, n_k);
    total += kh;
  }
  if (v[TV_LOSS_KEYPOINT_AFFINITY].p) {
    out[2] = p.l_aff * (float)d[6];
    out[16 + TV_LOSS_KEYPOINT_AFFINITY] = p.l_aff;
    total += out[2];
  }
  out[4] = __fdiv_rn(p.l_size * (float)s[ObjSize], n_valid);
  total += out[4];
  out[9] = __fdiv_rn((float)s[ObjErrSum], (float)s[ObjErrCount]);
  out[10] = err_max;
  out[3] = __fdiv_rn(p.l_offset * (float)s[ObjOffset], n_valid);
  total += out[3];
  for (int a = 0; a < 3; ++a) {
    if (!v[TV_LOSS_ROLL_BIN + 2 * a].p) continue;
    // lambda * (valid * angle_loss(...).sum()).sum() / n_valid: the sum over all objects, times the count
    out[5 + a] = __fdiv_rn(p.l_angle * (count * (float)s[ObjRoll + a]), n_valid);
    total += out[5 + a];
  }
  if (v[TV_LOSS_DEPTH].p) {
    out[8] = __fdiv_rn(p.l_depth * (float)s[ObjDepth], n_valid);
    total += out[8];
  }
  out[0] = total;
  for (int i = TV_LOSS_SIZE; i < TV_LOSS_TENSORS; ++i) out[16 + i] = v[i].p ? 1.f : 0.f;
}

// backward: a stored gradient (a dense buffer of n elements) times the device-side fp32 scalar *s, in place.
// The product is formed in fp32 from the stored value and the unrounded scalar, then rounded once.
template <typename T>
__global__ __launch_bounds__(kThreads) void scale(T* __restrict__ g, long long n, const float* __restrict__ s) {
  constexpr int V = 16 / (int)sizeof(T);
  const float f = *s;
  const long long i = ((long long)blockIdx.x * kThreads + threadIdx.x) * V;
  if (i + V <= n) {
    Vec<T, V> v = *reinterpret_cast<Vec<T, V>*>(g + i);
#pragma unroll
    for (int j = 0; j < V; ++j) v.e[j] = from_f<T>(to_f<T>(v.e[j]) * f);
    *reinterpret_cast<Vec<T, V>*>(g + i) = v;
  } else {
    for (long long k = i; k < n; ++k) g[k] = from_f<T>(to_f<T>(g[k]) * f);
  }
}

template <typename T>
static void launch_scale(void* g, long long n, const float* s, hipStream_t st) {
  const long long per_block = (long long)kThreads * (16 / (int)sizeof(T));
  hipLaunchKernelGGL(scale<T>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kThreads), 0, st,
                     reinterpret_cast<T*>(g), n, s);
}

// ---- host --------------------------------------------------------------------------------------

static int fail(const char* msg) {
  set_error(std::string("centernet_loss: ") + msg);
  return 1;
}

static int ndim_of(int i) { return i == TV_LOSS_KEYPOINT_AFFINITY ? 5 : 4; }

// a present tensor's view is four-element aligned and contiguous over (y, x)
static bool vector_ok(const tv_loss_tensor& t, int i, int W, int esize) {
  const int n = ndim_of(i);
  for (const int64_t* st : {t.stride, t.grad ? t.grad_stride : t.stride}) {
    if (st[n - 1] != 1 || st[n - 2] != W) return false;
    for (int k = 0; k < n - 2; ++k)
      if (st[k] % 4) return false;
  }
  const uintptr_t mask = (uintptr_t)(4 * esize - 1);
  return !((uintptr_t)t.data & mask) && !((uintptr_t)t.grad & mask);
}

struct Checked {
  Params p;
  bool vec;
  size_t dense_floats, bytes;
};

// every argument check of the three entry points; fills the kernels' parameters
static int check(const tv_loss_desc* d, Checked* c) {
  if (!d) return fail("null description");
  if (d->dtype != F32 && d->dtype != F16 && d->dtype != BF16) return fail("dtype must be TV_F32, TV_F16 or TV_BF16");
  if (d->B < 1) return fail("B must be >= 1");
  if (d->n_objects < 0 || d->n_instances < 0 || d->n_labels < 1 || d->n_keypoints < 0) return fail("negative count");
  if (d->in_h < 1 || d->in_w < 1 || d->downsample_ratio < 1) return fail("bad input size or downsample ratio");
  const int H = d->in_h / d->downsample_ratio, W = d->in_w / d->downsample_ratio;
  if (H < 1 || W < 1) return fail("empty output map");
  const tv_loss_tensor* t = d->tensor;
  if (!t[TV_LOSS_HEATMAP].data || !t[TV_LOSS_SIZE].data || !t[TV_LOSS_OFFSET].data)
    return fail("the heatmap, size and offset heads are required");
  if (t[TV_LOSS_KEYPOINT_AFFINITY].data && !t[TV_LOSS_KEYPOINT_HEATMAP].data)
    return fail("the keypoint affinity needs the keypoint heatmap");
  const bool kp = t[TV_LOSS_KEYPOINT_HEATMAP].data != nullptr;
  if (kp && d->n_keypoints < 1) return fail("the keypoint heads need n_keypoints >= 1");
  for (int a = 0; a < 3; ++a)
    if (!t[TV_LOSS_ROLL_BIN + 2 * a].data != !t[TV_LOSS_ROLL_OFFSET + 2 * a].data)
      return fail("an angle's bin and offset heads go together");
  bool any_grad = false;
  for (int i = 0; i < TV_LOSS_TENSORS; ++i) any_grad = any_grad || (t[i].data && t[i].grad);
  for (int i = 0; i < TV_LOSS_TENSORS; ++i) {
    if (!t[i].data) continue;
    if (any_grad && !t[i].grad) return fail("gradient buffers for every present head, or for none");
    for (int k = 0; k < ndim_of(i); ++k)
      if (t[i].stride[k] < 0 || (t[i].grad && t[i].grad_stride[k] < 0)) return fail("negative stride");
  }
  if (d->n_objects && (!d->valid || !d->label || !d->center || !d->size)) return fail("null truth pointer");
  if (d->n_objects && ((t[TV_LOSS_ROLL_BIN].data && !d->roll) || (t[TV_LOSS_PITCH_BIN].data && !d->pitch) ||
                       (t[TV_LOSS_YAW_BIN].data && !d->yaw) || (t[TV_LOSS_DEPTH].data && !d->depth)))
    return fail("null truth pointer for a present head");
  if ((t[TV_LOSS_ROLL_BIN].data || t[TV_LOSS_PITCH_BIN].data || t[TV_LOSS_YAW_BIN].data) && !d->angle_range)
    return fail("null angle_range");
  if (kp && d->n_instances &&
      (!d->keypoint_valid || !d->keypoint_label || !d->keypoint_center || !d->keypoint_object_index || !d->center))
    return fail("null keypoint truth pointer");
  if (!(d->focal_alpha >= 1.0) || !(d->focal_beta >= 1.0)) return fail("focal alpha and beta must be >= 1");

  Params& p = c->p;
  p = Params{};
  p.t.valid = d->valid; p.t.label = reinterpret_cast<const long long*>(d->label); p.t.center = d->center;
  p.t.kvalid = d->keypoint_valid; p.t.klabel = reinterpret_cast<const long long*>(d->keypoint_label);
  p.t.kcenter = d->keypoint_center; p.t.kobj = reinterpret_cast<const long long*>(d->keypoint_object_index);
  p.t.n_obj = d->n_objects; p.t.n_inst = d->n_instances;
  p.t.in_h = d->in_h; p.t.in_w = d->in_w; p.t.ratio = d->downsample_ratio; p.t.H = H; p.t.W = W;
  c->vec = (H * W) % 4 == 0;
  for (int i = 0; i < TV_LOSS_TENSORS; ++i) {
    p.v[i].p = t[i].data;
    p.v[i].g = t[i].data ? t[i].grad : nullptr;
    for (int k = 0; k < 5; ++k) { p.v[i].st[k] = t[i].stride[k]; p.v[i].gst[k] = t[i].grad_stride[k]; }
    if (t[i].data && i <= TV_LOSS_KEYPOINT_AFFINITY) c->vec = c->vec && vector_ok(t[i], i, W, dtype_size(d->dtype));
  }
  p.size = d->size; p.roll = d->roll; p.pitch = d->pitch; p.yaw = d->yaw; p.depth = d->depth;
  p.angle_range = d->angle_range;
  p.B = d->B; p.L = d->n_labels; p.K = kp ? d->n_keypoints : 0;
  const int per_block = kThreads * (c->vec ? 4 : 1);
  p.gx = (H * W + per_block - 1) / per_block;
  p.den_heat = targets::den_of(d->keypoint_heatmap_sigma < 0.1 ? 0.1 : d->keypoint_heatmap_sigma);  // loss.py:58-62
  p.den_kp = targets::den_of(d->keypoint_heatmap_sigma);
  p.den_aff = targets::den_of(d->keypoint_affinity_sigma);
  p.alpha = (float)d->focal_alpha; p.beta = (float)d->focal_beta;
  const double two_pi = 6.283185307179586;
  for (int i = 0; i < 2; ++i) {  // angle_in_range's range_min % (2 pi), range_max % (2 pi) as Python floats
    const double lo = d->bins[i][1] - two_pi * std::floor(d->bins[i][1] / two_pi);
    const double hi = d->bins[i][2] - two_pi * std::floor(d->bins[i][2] / two_pi);
    p.bin_center[i] = (float)d->bins[i][0]; p.bin_min[i] = (float)lo; p.bin_max[i] = (float)hi;
    p.bin_wraps[i] = !(lo < hi);
  }
  p.l_kh = (float)d->lambda_keypoint_heatmap; p.l_aff = (float)d->lambda_keypoint_affinity;
  p.l_size = (float)d->lambda_size; p.l_offset = (float)d->lambda_offset;
  p.l_angle = (float)d->lambda_angle; p.l_depth = (float)d->lambda_depth;
  c->dense_floats = (size_t)p.B * (p.L + p.K) * p.gx * kDenseF;
  c->bytes = (c->dense_floats + (size_t)p.B * kObjF) * sizeof(float);
  return 0;
}

static int check_ws(const tv_loss_desc* d, const void* ws, int64_t ws_bytes, Checked* c) {
  const int rc = check(d, c);
  if (rc) return rc;
  if (!ws || ws_bytes < (int64_t)c->bytes) return fail("null or too small workspace");
  c->p.dense_part = const_cast<float*>(reinterpret_cast<const float*>(ws));
  c->p.obj_part = c->p.dense_part + c->dense_floats;
  return 0;
}

template <typename T>
static void launch_dense(const Checked& c, hipStream_t s) {
  const Params& p = c.p;
  const dim3 grid((unsigned)p.gx, (unsigned)(p.L + p.K + 1), (unsigned)p.B), block(kThreads);
  if (c.vec) hipLaunchKernelGGL((dense<T, 4>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((dense<T, 1>), grid, block, 0, s, p);
}

}  // namespace loss

int centernet_loss_workspace_size(const tv_loss_desc* d, long long* bytes) {
  loss::Checked c;
  if (!bytes) return loss::fail("null bytes");
  const int rc = loss::check(d, &c);
  if (rc) return rc;
  *bytes = (long long)c.bytes;
  return 0;
}

int launch_centernet_loss_dense(const tv_loss_desc* d, void* ws, long long ws_bytes, hipStream_t s) {
  loss::Checked c;
  const int rc = loss::check_ws(d, ws, ws_bytes, &c);
  if (rc) return rc;
  if (c.p.L + c.p.K + 1 > 65535 || c.p.B > 65535) return loss::fail("too many planes or samples for one grid");
  if (d->dtype == F32) loss::launch_dense<float>(c, s);
  else if (d->dtype == F16) loss::launch_dense<_Float16>(c, s);
  else loss::launch_dense<__bf16>(c, s);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_centernet_loss_objects(const tv_loss_desc* d, void* ws, long long ws_bytes, hipStream_t s) {
  loss::Checked c;
  const int rc = loss::check_ws(d, ws, ws_bytes, &c);
  if (rc) return rc;
  const dim3 grid((unsigned)((c.p.B + 63) / 64)), block(64);
  if (d->dtype == F32) hipLaunchKernelGGL(loss::objects<float>, grid, block, 0, s, c.p);
  else if (d->dtype == F16) hipLaunchKernelGGL(loss::objects<_Float16>, grid, block, 0, s, c.p);
  else hipLaunchKernelGGL(loss::objects<__bf16>, grid, block, 0, s, c.p);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_centernet_loss_scale(void* grad, int dtype, long long n, const float* scale, hipStream_t s) {
  if (dtype != F32 && dtype != F16 && dtype != BF16) return loss::fail("dtype must be TV_F32, TV_F16 or TV_BF16");
  if (!grad || !scale || n < 0 || ((uintptr_t)grad & 15)) return loss::fail("scale: null, misaligned or negative");
  if (n >= (1ll << 40)) return loss::fail("scale: too many elements for one grid");
  if (n == 0) return 0;
  if (dtype == F32) loss::launch_scale<float>(grad, n, scale, s);
  else if (dtype == F16) loss::launch_scale<_Float16>(grad, n, scale, s);
  else loss::launch_scale<__bf16>(grad, n, scale, s);
  TV_HIP(hipGetLastError());
  return 0;
}

int launch_centernet_loss_finalize(const tv_loss_desc* d, const void* ws, long long ws_bytes, float* out,
                                   hipStream_t s) {
  loss::Checked c;
  const int rc = loss::check_ws(d, ws, ws_bytes, &c);
  if (rc) return rc;
  if (!out) return loss::fail("null out");
  hipLaunchKernelGGL(loss::finalize, dim3(1), dim3(loss::kThreads), 0, s, c.p, out);
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
