// The YOLACT training loss with its gradients (reference yolact/model/loss.py:8-124, boxes.py:45-103),
// gfx950. The contract is tv_yolact_loss_* in include/tauv_vision_amd.h.
//
// The reference loops in Python over the samples (classification, box) and over every positive anchor
// (mask: a host round trip, two interpolations of the full-resolution seg map, a meshgrid and a
// [P] x [P, h, w] product each), and autograd replays all of it. Here, whatever B, T and the positive count:
//   match       one thread per (sample, anchor): iou_matrix's fp32 operation sequence without contraction,
//               times truth_valid, max over T (lowest index wins), the two threshold flags, and the
//               background softmax probability, the key of the hard-negative mining.
//   select      one workgroup per sample: the positives compacted in anchor order into the sample's list,
//               k = min(ratio * n_positive, n_negative), an exact radix select (four 8-bit passes over the
//               keys' bits, integer LDS counters) of the k-th smallest key among the negatives, then one
//               ordered pass that takes the keys below it and the ties by anchor index.
//   anchors     one thread per (sample, anchor): cross-entropy at the selected anchors, smooth-L1 against
//               box_encode of the matched truth at the positives, both gradients (every element written
//               once, zeros included), and the zero rows of d mask_coeff at the non-positives.
//   mask_sums   one workgroup per (sample, truth): the sum of the bilinearly resized truth mask.
//   mask        one workgroup per (sample, tile of 256 prototype pixels, chunk of 32 prototypes): a thread
//               keeps its pixel's 32 prototype values, its four seg-map taps and its validity in registers
//               and walks the sample's positive list: logit, clamped sigmoid, weighted BCE, dL/dlogit;
//               d prototype accumulates in 32 registers and is stored once. No truth plane is stored.
//   mask_coeff  one wavefront per positive walks the pixels of the matched truth's box, forms the same
//               dL/dlogit and reduces d mask_coeff over its 64 lanes by a butterfly: no partial sums per
//               tile (their number, B * A * tiles * P, cannot be sized without the positive count).
//   finalize    one workgroup sums the partial sums in a fixed order, in double, and writes the three
//               terms, the total, the counts and each gradient tensor's factor.
// No float atomics, no waiting between workgroups, no grid that depends on a device-side count: a call's
// bits depend on its inputs alone. Every index read from memory (match index, list entry, count, class)
// is clamped to its range before it is used.
#include "conv_common.h"

#include "../../include/tauv_vision_amd.h"

namespace tv {
namespace yloss {

constexpr int kThreads = 256;
constexpr int kSelect = 1024;  // threads of a select workgroup
constexpr int kPC = 32;        // prototypes a mask thread holds in registers
constexpr int kCoeffGroups = 256;  // mask_coeff workgroups per (sample, chunk) at most: 1024 wavefronts

struct Params {
  int B, A, C, P, T, h, w, in_h, in_w, seg_size, ratio;
  float pos_th, neg_th, var0, var1, scale_h, scale_w;
  const float *cls, *box, *coeff, *anchor, *proto;
  float *gcls, *gbox, *gcoeff, *gproto;
  long long cls_st[3], box_st[3], coeff_st[3], anchor_st[2], proto_st[4];
  long long gcls_st[3], gbox_st[3], gcoeff_st[3], gproto_st[4];
  const unsigned char* valid;  // [B][T]
  const long long* tcls;       // [B][T]
  const float* tbox;           // [B][T][4]
  const void* seg;             // [B][in_h][in_w], seg_size bytes each
  const unsigned char* img_valid;
  int* match;                  // [B][A]
  unsigned char *positive, *negative, *selected;
  // workspace
  float* key;          // [B][A]
  int* poslist;        // [B][A]
  int* counts;         // [B][4]: positives, negatives, mined negatives
  float* tsum;         // [B][T]
  float* anchor_part;  // [B][anchor_blocks][2]
  float* mask_part;    // [B][tiles]
  int anchor_blocks, tiles, chunks;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// sum over a 256-thread workgroup in a fixed order: 64-lane butterfly, then the four waves in wave order
__device__ __forceinline__ float block_sum(float v, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

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

// ---- match -------------------------------------------------------------------------------------

// max and sum of exp of one anchor's logits
__device__ __forceinline__ void softmax_stats(const float* l, long long st, int C, float& m, float& sum) {
  m = l[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c * st]);
  sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(l[c * st] - m);
}

// grid (ceil(A / 256), B)
__global__ __launch_bounds__(kThreads) void match(const Params p) {
  const int a = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  if (a >= p.A) return;
  const float* an = p.anchor + a * p.anchor_st[0];
  const float ay = an[0], ax = an[p.anchor_st[1]], ah = an[2 * p.anchor_st[1]], aw = an[3 * p.anchor_st[1]];
  // box_to_corners, iou_matrix (boxes.py:15-27, 64-85): each operation rounded on its own
  const float a0 = __fsub_rn(ay, __fdiv_rn(ah, 2.f)), a1 = __fsub_rn(ax, __fdiv_rn(aw, 2.f));
  const float a2 = __fadd_rn(ay, __fdiv_rn(ah, 2.f)), a3 = __fadd_rn(ax, __fdiv_rn(aw, 2.f));
  const float area_a = __fmul_rn(ah, aw);
  float best = 0.f;
  int idx = 0;
  for (int t = 0; t < p.T; ++t) {
    const float* tb = p.tbox + ((size_t)b * p.T + t) * 4;
    const float b0 = __fsub_rn(tb[0], __fdiv_rn(tb[2], 2.f)), b1 = __fsub_rn(tb[1], __fdiv_rn(tb[3], 2.f));
    const float b2 = __fadd_rn(tb[0], __fdiv_rn(tb[2], 2.f)), b3 = __fadd_rn(tb[1], __fdiv_rn(tb[3], 2.f));
    const float ih = fmaxf(__fsub_rn(fminf(a2, b2), fmaxf(a0, b0)), 0.f);
    const float iw = fmaxf(__fsub_rn(fminf(a3, b3), fmaxf(a1, b1)), 0.f);
    const float inter = __fmul_rn(ih, iw);
    const float uni = __fsub_rn(__fadd_rn(area_a, __fmul_rn(tb[2], tb[3])), inter);
    const float v = __fmul_rn(__fdiv_rn(inter, uni), p.valid[(size_t)b * p.T + t] ? 1.f : 0.f);
    // torch.max over T: the first maximum; a NaN wins and stays
    if (t == 0 || (best == best && (v > best || v != v))) {
      best = v;
      idx = t;
    }
  }
  const size_t ba = (size_t)b * p.A + a;
  p.match[ba] = idx;
  p.positive[ba] = best >= p.pos_th;  // NaN: neither
  p.negative[ba] = best <= p.neg_th;
  const float* l = p.cls + b * p.cls_st[0] + a * p.cls_st[1];
  float m, sum;
  softmax_stats(l, p.cls_st[2], p.C, m, sum);
  p.key[ba] = __fdiv_rn(expf(l[0] - m), sum);  // softmax(...)[:, 0]
}

// ---- select ------------------------------------------------------------------------------------

// exclusive prefix sum of v over the workgroup in thread order; total: the sum
__device__ __forceinline__ int block_scan(int v, int* lds, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int n = __shfl_up(inc, off, 64);
    if (lane >= off) inc += n;
  }
  __syncthreads();
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < kSelect / 64; ++i) {
    const int s = lds[i];
    base += i < wv ? s : 0;
    tot += s;
  }
  total = tot;
  return base + inc - v;
}

// grid (B)
__global__ __launch_bounds__(kSelect) void select(const Params p) {
  __shared__ int scan_lds[kSelect / 64];
  __shared__ int hist[256];
  __shared__ int s_bin, s_rem;
  const int b = blockIdx.x, tid = threadIdx.x, A = p.A;
  const size_t bA = (size_t)b * A;
  const unsigned char *pos = p.positive + bA, *neg = p.negative + bA;
  const unsigned* key = reinterpret_cast<const unsigned*>(p.key) + bA;  // probabilities: >= 0, ordered as integers

  int npos = 0, nneg = 0;
  for (int base = 0; base < A; base += kSelect) {
    const int a = base + tid;
    const int is_pos = a < A && pos[a], is_neg = a < A && neg[a];
    int tot;
    const int ex = block_scan(is_pos, scan_lds, tot);
    if (is_pos) p.poslist[bA + npos + ex] = a;  // npos + ex < the number of positives <= A
    npos += tot;
    nneg += __syncthreads_count(is_neg);
  }
  const long long want = (long long)p.ratio * npos;
  const int k = (int)(want < (long long)nneg ? want : (long long)nneg);  // the departure: min(k, n_negative)

  // the k-th smallest key among the negatives (0 < k < nneg), by its bits from the top byte down
  unsigned prefix = 0, mask = 0;
  int rem = k;
  if (k > 0 && k < nneg) {
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      if (tid == 0) { s_bin = 255; s_rem = 0; }
      __syncthreads();
      for (int a = tid; a < A; a += kSelect)
        if (neg[a] && (key[a] & mask) == prefix) atomicAdd(&hist[(key[a] >> shift) & 255u], 1);
      __syncthreads();
      if (tid == 0) {
        int cum = 0;
        for (int bin = 0; bin < 256; ++bin) {
          const int c = hist[bin];
          if (cum + c >= rem) { s_bin = bin; s_rem = rem - cum; break; }
          cum += c;
        }
      }
      __syncthreads();
      prefix |= (unsigned)s_bin << shift;
      mask |= 255u << shift;
      rem = s_rem;
      __syncthreads();
    }
  }
  // keys below the k-th, then `rem` of its ties in anchor order; k == nneg takes every negative
  const bool all = k > 0 && k >= nneg, none = k <= 0;
  int ties = 0;
  for (int base = 0; base < A; base += kSelect) {
    const int a = base + tid;
    const bool live = a < A, is_neg = live && neg[a];
    const unsigned kv = live ? key[a] : 0u;
    const int tie = is_neg && !all && !none && kv == prefix;
    int tot;
    const int ex = block_scan(tie, scan_lds, tot);
    const bool mined = is_neg && !none && (all || kv < prefix || (tie && ties + ex < rem));
    if (live) p.selected[bA + a] = pos[a] || mined;
    ties += tot;
  }
  if (tid == 0) {
    int* c = p.counts + (size_t)b * 4;
    c[0] = npos; c[1] = nneg; c[2] = k > 0 ? k : 0; c[3] = 0;
  }
}

// ---- anchors -----------------------------------------------------------------------------------

// grid (anchor_blocks, B)
__global__ __launch_bounds__(kThreads) void anchors(const Params p) {
  __shared__ float lds[4];
  const int a = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  float cls_sum = 0.f, box_sum = 0.f;
  if (a < p.A) {
    const size_t ba = (size_t)b * p.A + a;
    const bool pos = p.positive[ba], sel = p.selected[ba];
    const int t = clampi(p.match[ba], 0, p.T - 1);
    // cross-entropy (log-softmax, max-subtracted) against the matched class at positives, 0 elsewhere
    const float* l = p.cls + b * p.cls_st[0] + a * p.cls_st[1];
    float* g = p.gcls ? p.gcls + b * p.gcls_st[0] + a * p.gcls_st[1] : nullptr;
    if (sel) {
      const int target = pos ? clampi((int)p.tcls[(size_t)b * p.T + t], 0, p.C - 1) : 0;
      float m, sum;
      softmax_stats(l, p.cls_st[2], p.C, m, sum);
      cls_sum = logf(sum) - (l[target * p.cls_st[2]] - m);
      if (g)
        for (int c = 0; c < p.C; ++c)
          g[c * p.gcls_st[2]] = __fdiv_rn(expf(l[c * p.cls_st[2]] - m), sum) - (c == target ? 1.f : 0.f);
    } else if (g) {
      for (int c = 0; c < p.C; ++c) g[c * p.gcls_st[2]] = 0.f;
    }
    // smooth-L1 (beta 1) against box_encode(truth_box[match], anchor) at positives (boxes.py:45-52)
    float* gb = p.gbox ? p.gbox + b * p.gbox_st[0] + a * p.gbox_st[1] : nullptr;
    if (pos) {
      const float* e = p.box + b * p.box_st[0] + a * p.box_st[1];
      const float* an = p.anchor + a * p.anchor_st[0];
      const float* tb = p.tbox + ((size_t)b * p.T + t) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float asz = an[(2 + (j & 1)) * p.anchor_st[1]];
        const float target = j < 2 ? __fdiv_rn(tb[j] - an[j * p.anchor_st[1]], p.var0 * asz)
                                   : __fdiv_rn(logf(__fdiv_rn(tb[j], asz)), p.var1);
        const float d = e[j * p.box_st[2]] - target, ad = fabsf(d);
        box_sum += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
        if (gb) gb[j * p.gbox_st[2]] = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
      }
    } else {
      if (gb)
        for (int j = 0; j < 4; ++j) gb[j * p.gbox_st[2]] = 0.f;
      if (p.gcoeff) {  // positives' rows are mask_coeff's
        float* gc = p.gcoeff + b * p.gcoeff_st[0] + a * p.gcoeff_st[1];
        for (int i = 0; i < p.P; ++i) gc[i * p.gcoeff_st[2]] = 0.f;
      }
    }
  }
  cls_sum = block_sum(cls_sum, lds);
  box_sum = block_sum(box_sum, lds);
  if (threadIdx.x == 0) {
    float* o = p.anchor_part + ((size_t)b * p.anchor_blocks + blockIdx.x) * 2;
    o[0] = cls_sum;
    o[1] = box_sum;
  }
}

// ---- mask --------------------------------------------------------------------------------------

// the seg map's value at (b, y, x) if it is a truth index, else -1
__device__ __forceinline__ int seg_at(const Params& p, int b, int y, int x) {
  const size_t i = ((size_t)b * p.in_h + y) * p.in_w + x;
  long long v;
  if (p.seg_size == 1) v = reinterpret_cast<const unsigned char*>(p.seg)[i];
  else if (p.seg_size == 2) v = reinterpret_cast<const short*>(p.seg)[i];
  else if (p.seg_size == 4) v = reinterpret_cast<const int*>(p.seg)[i];
  else v = reinterpret_cast<const long long*>(p.seg)[i];
  return v >= 0 && v < p.T ? (int)v : -1;
}

// upsample_bilinear2d's source index and weights (align_corners false) along one axis
__device__ __forceinline__ void source(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f), 0.f);
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(__fsub_rn(s, (float)i0), 0.f), 1.f);
  l0 = __fsub_rn(1.f, l1);
}

// a prototype pixel's view of the truth: four seg-map taps with their weights, and the nearest validity
struct Pixel {
  int s00, s01, s10, s11;
  float ly0, ly1, lx0, lx1, valid;
};
__device__ __forceinline__ Pixel pixel_of(const Params& p, int b, int y, int x) {
  Pixel q;
  int y0, y1, x0, x1;
  source(p.scale_h, y, p.in_h, y0, y1, q.ly0, q.ly1);
  source(p.scale_w, x, p.in_w, x0, x1, q.lx0, q.lx1);
  q.s00 = seg_at(p, b, y0, x0); q.s01 = seg_at(p, b, y0, x1);
  q.s10 = seg_at(p, b, y1, x0); q.s11 = seg_at(p, b, y1, x1);
  // upsample_nearest2d: min(floor(dst * scale), in - 1)
  const int ny = min((int)floorf(__fmul_rn((float)y, p.scale_h)), p.in_h - 1);
  const int nx = min((int)floorf(__fmul_rn((float)x, p.scale_w)), p.in_w - 1);
  q.valid = p.img_valid[((size_t)b * p.in_h + ny) * p.in_w + nx] ? 1.f : 0.f;
  return q;
}
// (truth_seg_map == t) resized to the pixel
__device__ __forceinline__ float resized(const Pixel& q, int t) {
  const float v00 = q.s00 == t, v01 = q.s01 == t, v10 = q.s10 == t, v11 = q.s11 == t;
  return __fadd_rn(__fmul_rn(q.ly0, __fadd_rn(__fmul_rn(q.lx0, v00), __fmul_rn(q.lx1, v01))),
                   __fmul_rn(q.ly1, __fadd_rn(__fmul_rn(q.lx0, v10), __fmul_rn(q.lx1, v11))));
}

// grid (T, B): the sum of the resized truth mask of truth t
__global__ __launch_bounds__(kThreads) void mask_sums(const Params p) {
  __shared__ double lds[kThreads];
  const int t = blockIdx.x, b = blockIdx.y, n = p.h * p.w;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int y = i / p.w, x = i - y * p.w;
    acc += resized(pixel_of(p, b, y, x), t);
  }
  const double s = block_sum_d((double)acc, lds);
  if (threadIdx.x == 0) p.tsum[(size_t)b * p.T + t] = (float)s;
}

// box_to_mask's edges (boxes.py:93-98) of truth (b, t) on the prototype grid
struct Edges {
  float left, right, top, bottom;
};
__device__ __forceinline__ Edges edges_of(const Params& p, int b, int t) {
  const float* tb = p.tbox + ((size_t)b * p.T + t) * 4;
  const float cy = __fmul_rn(tb[0], (float)p.h), cx = __fmul_rn(tb[1], (float)p.w);
  const float bh = __fmul_rn(tb[2], (float)p.h), bw = __fmul_rn(tb[3], (float)p.w);
  Edges e;
  e.left = __fsub_rn(cx, __fdiv_rn(bw, 2.f));
  e.right = __fadd_rn(cx, __fdiv_rn(bw, 2.f));
  e.top = __fsub_rn(cy, __fdiv_rn(bh, 2.f));
  e.bottom = __fadd_rn(cy, __fdiv_rn(bh, 2.f));
  return e;
}
__device__ __forceinline__ bool inside(const Edges& e, int y, int x) {
  const float yf = (float)y, xf = (float)x;
  return xf >= e.left && xf <= e.right && yf >= e.top && yf <= e.bottom;
}

// One pixel of one positive's mask term: logit z, resized truth tm, weight wgt = box mask * validity / the
// resized mask's sum. Adds the weighted BCE to loss and returns dL/dz. The clamps (loss.py:84, 97) pass the
// gradient on the closed interval [1e-4, 1 - 1e-4] of the sigmoid.
__device__ __forceinline__ float mask_cell(float z, float tm, float wgt, float& loss) {
  const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
  const float s = __fdiv_rn(1.f, 1.f + expf(-z));
  const float m = fminf(fmaxf(s, lo), hi), tc = fminf(fmaxf(tm, lo), hi);
  loss += wgt * -(tc * logf(m) + (1.f - tc) * logf(1.f - m));
  const float dm = s >= lo && s <= hi ? __fdiv_rn(1.f - tc, 1.f - m) - __fdiv_rn(tc, m) : 0.f;
  return wgt * dm * ((1.f - s) * s);
}

// this chunk's coefficients of anchor (b, a), zero past P
__device__ __forceinline__ void load_coeff(const Params& p, int b, int a, int p0, float (&cf)[kPC]) {
  const float* c = p.coeff + b * p.coeff_st[0] + a * p.coeff_st[1];
#pragma unroll
  for (int i = 0; i < kPC; ++i) cf[i] = p0 + i < p.P ? c[(p0 + i) * p.coeff_st[2]] : 0.f;
}
// this chunk's prototype values at pixel (b, y, x), zero past P
__device__ __forceinline__ void load_proto(const Params& p, int b, int y, int x, int p0, float (&pr)[kPC]) {
  const float* q = p.proto + b * p.proto_st[0] + y * p.proto_st[2] + x * p.proto_st[3];
#pragma unroll
  for (int i = 0; i < kPC; ++i) pr[i] = p0 + i < p.P ? q[(p0 + i) * p.proto_st[1]] : 0.f;
}
// the logit: from the registers when one chunk holds every prototype, else over all of them from memory
template <bool SINGLE>
__device__ __forceinline__ float logit_of(const Params& p, int b, int a, int y, int x, const float (&cf)[kPC],
                                          const float (&pr)[kPC]) {
  float z = 0.f;
  if (SINGLE) {
#pragma unroll
    for (int i = 0; i < kPC; ++i) z = fmaf(cf[i], pr[i], z);
  } else {
    const float* c = p.coeff + b * p.coeff_st[0] + a * p.coeff_st[1];
    const float* q = p.proto + b * p.proto_st[0] + y * p.proto_st[2] + x * p.proto_st[3];
    for (int i = 0; i < p.P; ++i) z = fmaf(c[i * p.coeff_st[2]], q[i * p.proto_st[1]], z);
  }
  return z;
}

// grid (tiles, chunks, B)
template <bool SINGLE>
__global__ __launch_bounds__(kThreads) void mask(const Params p) {
  __shared__ float lds[4];
  const int b = blockIdx.z, p0 = blockIdx.y * kPC, n = p.h * p.w;
  const int first = blockIdx.x * kThreads, pix = first + threadIdx.x;
  const bool live = pix < n;
  const int y = live ? pix / p.w : 0, x = live ? pix - y * p.w : 0;
  const float y_first = (float)(first / p.w), y_last = (float)(min(first + kThreads - 1, n - 1) / p.w);
  float pr[kPC], acc[kPC];
  load_proto(p, b, y, x, p0, pr);
#pragma unroll
  for (int i = 0; i < kPC; ++i) acc[i] = 0.f;
  const Pixel q = pixel_of(p, b, y, x);
  const size_t bA = (size_t)b * p.A;
  const int npos = clampi(p.counts[(size_t)b * 4], 0, p.A);
  float loss = 0.f;
  for (int i = 0; i < npos; ++i) {
    const int a = clampi(p.poslist[bA + i], 0, p.A - 1);
    const int t = clampi(p.match[bA + a], 0, p.T - 1);
    const float sum = p.tsum[(size_t)b * p.T + t];
    if (sum == 0.f) continue;  // loss.py:93-94
    const Edges e = edges_of(p, b, t);
    if (y_last < e.top || y_first > e.bottom) continue;  // no row of this tile meets the box
    const float wgt = live && inside(e, y, x) ? q.valid : 0.f;
    if (wgt != 0.f) {
      float cf[kPC];
      load_coeff(p, b, a, p0, cf);
      const float g = mask_cell(logit_of<SINGLE>(p, b, a, y, x, cf, pr), resized(q, t), __fdiv_rn(wgt, sum), loss);
#pragma unroll
      for (int j = 0; j < kPC; ++j) acc[j] = fmaf(g, cf[j], acc[j]);
    }
  }
  if (p.gproto && live) {
    float* g = p.gproto + b * p.gproto_st[0] + y * p.gproto_st[2] + x * p.gproto_st[3];
#pragma unroll
    for (int i = 0; i < kPC; ++i)
      if (p0 + i < p.P) g[(p0 + i) * p.gproto_st[1]] = acc[i];
  }
  if (blockIdx.y == 0) {
    loss = block_sum(loss, lds);
    if (threadIdx.x == 0) p.mask_part[(size_t)b * p.tiles + blockIdx.x] = loss;
  }
}

// grid (groups, chunks, B): wavefront `slot` of the (sample, chunk) takes positives slot, slot + slots, ...
template <bool SINGLE>
__global__ __launch_bounds__(kThreads) void mask_coeff(const Params p) {
  const int b = blockIdx.z, p0 = blockIdx.y * kPC, lane = threadIdx.x & 63;
  const int slot = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6));
  const int slots = gridDim.x * (kThreads / 64);
  const size_t bA = (size_t)b * p.A;
  const int npos = clampi(p.counts[(size_t)b * 4], 0, p.A);
  for (int i = slot; i < npos; i += slots) {
    const int a = clampi(p.poslist[bA + i], 0, p.A - 1);
    const int t = clampi(p.match[bA + a], 0, p.T - 1);
    const float sum = p.tsum[(size_t)b * p.T + t];
    float dc[kPC];
#pragma unroll
    for (int j = 0; j < kPC; ++j) dc[j] = 0.f;
    if (sum != 0.f) {
      const Edges e = edges_of(p, b, t);
      // the rows and columns the box can reach (a NaN edge leaves the whole axis; inside() decides)
      const int r0 = e.top > 0.f ? (e.top < (float)p.h ? (int)e.top : p.h) : 0;
      const int r1 = e.bottom < 0.f ? -1 : (e.bottom < (float)(p.h - 1) ? (int)e.bottom : p.h - 1);
      const int c0 = e.left > 0.f ? (e.left < (float)p.w ? (int)e.left : p.w) : 0;
      const int c1 = e.right < 0.f ? -1 : (e.right < (float)(p.w - 1) ? (int)e.right : p.w - 1);
      const int cw = c1 - c0 + 1, cells = r1 >= r0 && c1 >= c0 ? (r1 - r0 + 1) * cw : 0;
      float cf[kPC];
      load_coeff(p, b, a, p0, cf);
      float unused = 0.f;
      for (int c = lane; c < cells; c += 64) {
        const int y = r0 + c / cw, x = c0 + c % cw;  // 0 <= y < h, 0 <= x < w
        if (!inside(e, y, x)) continue;
        const Pixel q = pixel_of(p, b, y, x);
        if (q.valid == 0.f) continue;
        float pr[kPC];
        load_proto(p, b, y, x, p0, pr);
        const float g = mask_cell(logit_of<SINGLE>(p, b, a, y, x, cf, pr), resized(q, t), __fdiv_rn(q.valid, sum), unused);
#pragma unroll
        for (int j = 0; j < kPC; ++j) dc[j] = fmaf(g, pr[j], dc[j]);
      }
    }
    // over the 64 lanes, a butterfly per prototype; lane j stores prototype p0 + j
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < kPC; ++j) {
      float v = dc[j];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      out = lane == j ? v : out;
    }
    if (lane < kPC && p0 + lane < p.P)
      p.gcoeff[b * p.gcoeff_st[0] + a * p.gcoeff_st[1] + (p0 + lane) * p.gcoeff_st[2]] = out;
  }
}

// ---- finalize ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void finalize(const Params p, float* __restrict__ out) {
  __shared__ double lds[kThreads];
  const int tid = threadIdx.x;
  double cls = 0, box = 0, msk = 0, npos = 0, nneg = 0, nsel = 0;
  for (int i = tid; i < p.B * p.anchor_blocks; i += kThreads) {
    cls += p.anchor_part[(size_t)i * 2];
    box += p.anchor_part[(size_t)i * 2 + 1];
  }
  for (int i = tid; i < p.B * p.tiles; i += kThreads) msk += p.mask_part[i];
  for (int b = tid; b < p.B; b += kThreads) {
    npos += p.counts[(size_t)b * 4];
    nneg += p.counts[(size_t)b * 4 + 1];
    nsel += p.counts[(size_t)b * 4] + p.counts[(size_t)b * 4 + 2];
  }
  cls = block_sum_d(cls, lds); box = block_sum_d(box, lds); msk = block_sum_d(msk, lds);
  npos = block_sum_d(npos, lds); nneg = block_sum_d(nneg, lds); nsel = block_sum_d(nsel, lds);
  if (tid != 0) return;
  // loss.py:54-57, 70-73, 117-120: the plain sums without a positive
  const float n = (float)npos, den = (float)((1.0 + (double)p.ratio) * npos);
  const bool any = npos > 0;
  const float l_cls = any ? __fdiv_rn((float)cls, den) : (float)cls;
  const float l_box = any ? __fdiv_rn((float)box, n) : (float)box;
  const float l_msk = any ? __fdiv_rn((float)msk, n) : (float)msk;
  for (int i = 0; i < 16; ++i) out[i] = 0.f;
  out[0] = __fadd_rn(__fadd_rn(l_cls, l_box), l_msk);
  out[1] = l_cls; out[2] = l_box; out[3] = l_msk;
  out[4] = n; out[5] = (float)nneg; out[6] = (float)nsel;
  // the factor of each gradient tensor: classification, box_encoding, mask_coeff, mask_prototype
  out[8] = any ? __fdiv_rn(1.f, den) : 1.f;
  out[9] = out[10] = out[11] = any ? __fdiv_rn(1.f, n) : 1.f;
}

// ---- host --------------------------------------------------------------------------------------

static int fail(const char* msg) {
  set_error(std::string("yolact_loss: ") + msg);
  return 1;
}

struct Checked {
  Params p;
  size_t off_poslist, off_counts, off_tsum, off_anchor, off_mask, words;
};

static bool nonneg(const int64_t* st, int n) {
  for (int i = 0; i < n; ++i)
    if (st[i] < 0) return false;
  return true;
}

// every argument check of the entry points; fills the kernels' parameters
static int check(const tv_yolact_loss_desc* d, Checked* c) {
  if (!d) return fail("null description");
  if (d->B < 1 || d->A < 1 || d->C < 1) return fail("B, A and C must be >= 1");
  if (d->T < 1) return fail("T must be >= 1 (the reference's max over no truth raises)");
  if (d->P < 1) return fail("P must be >= 1");
  if (d->h < 1 || d->w < 1 || d->in_h < 1 || d->in_w < 1) return fail("empty prototype grid or seg map");
  if (d->seg_itemsize != 1 && d->seg_itemsize != 2 && d->seg_itemsize != 4 && d->seg_itemsize != 8)
    return fail("seg_itemsize must be 1 (uint8), 2, 4 or 8 (signed)");
  if (d->negative_example_ratio < 0) return fail("negative_example_ratio must be >= 0");
  const long long lim = 1ll << 31;
  if ((long long)d->B * d->A >= lim || (long long)d->h * d->w >= lim || (long long)d->B * d->T >= lim ||
      (long long)d->B * d->in_h * d->in_w >= (1ll << 40))
    return fail("too many anchors, pixels or truths for 32-bit indices");
  if (d->B > 65535 || d->T > 65535 || (d->P + kPC - 1) / kPC > 65535) return fail("B, T or P too large for one grid");
  if (!d->classification || !d->box_encoding || !d->mask_coeff || !d->anchor || !d->mask_prototype)
    return fail("null prediction pointer");
  if (!d->truth_valid || !d->truth_classification || !d->truth_box || !d->truth_seg_map || !d->truth_img_valid)
    return fail("null truth pointer");
  if (!d->match_index || !d->positive || !d->negative || !d->selected) return fail("null state pointer");
  const int ng = !!d->grad_classification + !!d->grad_box_encoding + !!d->grad_mask_coeff + !!d->grad_mask_prototype;
  if (ng != 0 && ng != 4) return fail("gradient buffers for all four prediction tensors, or for none");
  if (!nonneg(d->classification_stride, 3) || !nonneg(d->box_encoding_stride, 3) || !nonneg(d->mask_coeff_stride, 3) ||
      !nonneg(d->anchor_stride, 2) || !nonneg(d->mask_prototype_stride, 4) || !nonneg(d->grad_classification_stride, 3) ||
      !nonneg(d->grad_box_encoding_stride, 3) || !nonneg(d->grad_mask_coeff_stride, 3) ||
      !nonneg(d->grad_mask_prototype_stride, 4))
    return fail("negative stride");

  Params& p = c->p;
  p = Params{};
  p.B = d->B; p.A = d->A; p.C = d->C; p.P = d->P; p.T = d->T; p.h = d->h; p.w = d->w;
  p.in_h = d->in_h; p.in_w = d->in_w; p.seg_size = d->seg_itemsize; p.ratio = d->negative_example_ratio;
  p.pos_th = (float)d->iou_pos_threshold; p.neg_th = (float)d->iou_neg_threshold;
  p.var0 = (float)d->box_variances[0]; p.var1 = (float)d->box_variances[1];
  p.scale_h = (float)d->in_h / (float)d->h;  // area_pixel_compute_scale<float>
  p.scale_w = (float)d->in_w / (float)d->w;
  p.cls = (const float*)d->classification; p.box = (const float*)d->box_encoding;
  p.coeff = (const float*)d->mask_coeff; p.anchor = (const float*)d->anchor; p.proto = (const float*)d->mask_prototype;
  p.gcls = (float*)d->grad_classification; p.gbox = (float*)d->grad_box_encoding;
  p.gcoeff = (float*)d->grad_mask_coeff; p.gproto = (float*)d->grad_mask_prototype;
  for (int i = 0; i < 3; ++i) {
    p.cls_st[i] = d->classification_stride[i]; p.box_st[i] = d->box_encoding_stride[i];
    p.coeff_st[i] = d->mask_coeff_stride[i]; p.gcls_st[i] = d->grad_classification_stride[i];
    p.gbox_st[i] = d->grad_box_encoding_stride[i]; p.gcoeff_st[i] = d->grad_mask_coeff_stride[i];
  }
  for (int i = 0; i < 2; ++i) p.anchor_st[i] = d->anchor_stride[i];
  for (int i = 0; i < 4; ++i) {
    p.proto_st[i] = d->mask_prototype_stride[i];
    p.gproto_st[i] = d->grad_mask_prototype_stride[i];
  }
  p.valid = (const unsigned char*)d->truth_valid; p.tcls = (const long long*)d->truth_classification;
  p.tbox = (const float*)d->truth_box; p.seg = d->truth_seg_map; p.img_valid = (const unsigned char*)d->truth_img_valid;
  p.match = d->match_index; p.positive = d->positive; p.negative = d->negative; p.selected = d->selected;
  p.anchor_blocks = (p.A + kThreads - 1) / kThreads;
  p.tiles = (p.h * p.w + kThreads - 1) / kThreads;
  p.chunks = (p.P + kPC - 1) / kPC;
  // the workspace, in 4-byte words: key, poslist, counts, tsum, anchor_part, mask_part
  const size_t BA = (size_t)p.B * p.A;
  c->off_poslist = BA;
  c->off_counts = 2 * BA;
  c->off_tsum = c->off_counts + (size_t)p.B * 4;
  c->off_anchor = c->off_tsum + (size_t)p.B * p.T;
  c->off_mask = c->off_anchor + (size_t)p.B * p.anchor_blocks * 2;
  c->words = c->off_mask + (size_t)p.B * p.tiles;
  return 0;
}

static int check_ws(const tv_yolact_loss_desc* d, const void* ws, long long ws_bytes, Checked* c) {
  const int rc = check(d, c);
  if (rc) return rc;
  if (!ws || ws_bytes < (long long)(c->words * 4) || ((uintptr_t)ws & 3)) return fail("null, misaligned or too small workspace");
  float* w = const_cast<float*>(reinterpret_cast<const float*>(ws));
  Params& p = c->p;
  p.key = w;
  p.poslist = reinterpret_cast<int*>(w + c->off_poslist);
  p.counts = reinterpret_cast<int*>(w + c->off_counts);
  p.tsum = w + c->off_tsum;
  p.anchor_part = w + c->off_anchor;
  p.mask_part = w + c->off_mask;
  return 0;
}

}  // namespace yloss

int yolact_loss_workspace_size(const tv_yolact_loss_desc* d, long long* bytes) {
  yloss::Checked c;
  if (!bytes) return yloss::fail("null bytes");
  const int rc = yloss::check(d, &c);
  if (rc) return rc;
  *bytes = (long long)(c.words * 4);
  return 0;
}

int launch_yolact_loss(int stage, const tv_yolact_loss_desc* d, void* ws, long long ws_bytes, float* out, hipStream_t s) {
  using namespace yloss;
  Checked c;
  const int rc = check_ws(d, ws, ws_bytes, &c);
  if (rc) return rc;
  const Params& p = c.p;
  constexpr int kT = yloss::kThreads;
  const dim3 block(kT);
  switch (stage) {
    case TV_YOLACT_LOSS_MATCH:
      hipLaunchKernelGGL(match, dim3(p.anchor_blocks, p.B), block, 0, s, p);
      break;
    case TV_YOLACT_LOSS_SELECT:
      hipLaunchKernelGGL(select, dim3(p.B), dim3(kSelect), 0, s, p);
      break;
    case TV_YOLACT_LOSS_ANCHORS:
      hipLaunchKernelGGL(anchors, dim3(p.anchor_blocks, p.B), block, 0, s, p);
      break;
    case TV_YOLACT_LOSS_MASK_SUMS:
      hipLaunchKernelGGL(mask_sums, dim3(p.T, p.B), block, 0, s, p);
      break;
    case TV_YOLACT_LOSS_MASK:
      if (p.chunks == 1) hipLaunchKernelGGL(mask<true>, dim3(p.tiles, 1, p.B), block, 0, s, p);
      else hipLaunchKernelGGL(mask<false>, dim3(p.tiles, p.chunks, p.B), block, 0, s, p);
      break;
    case TV_YOLACT_LOSS_MASK_COEFF: {
      if (!p.gcoeff) return fail("mask_coeff: no gradient buffers");
      const int groups = std::min(kCoeffGroups, (p.A + kT / 64 - 1) / (kT / 64));
      if (p.chunks == 1) hipLaunchKernelGGL(mask_coeff<true>, dim3(groups, 1, p.B), block, 0, s, p);
      else hipLaunchKernelGGL(mask_coeff<false>, dim3(groups, p.chunks, p.B), block, 0, s, p);
      break;
    }
    case TV_YOLACT_LOSS_FINALIZE:
      if (!out) return fail("null out");
      hipLaunchKernelGGL(finalize, dim3(1), block, 0, s, p, out);
      break;
    default:
      return fail("unknown stage");
  }
  TV_HIP(hipGetLastError());
  return 0;
}

}  // namespace tv
