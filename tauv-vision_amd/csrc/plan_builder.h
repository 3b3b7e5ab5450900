// The planners' shared toolkit: parameter registration, tensors, K-segments and the ops every
// network lowers to, written once over a Plan. A walker (planner*.cpp) derives from it and keeps
// only what is its network's: the module tree, the key names and the labels.
#pragma once
#include <utility>

#include "common.h"
#include "planner.h"

namespace tv {

struct PlanBuilder {
  Plan& P;
  // in front of every parameter key, weight / BatchNorm name and op label that goes through the
  // builder (a network appended under a parent module: "_backbone._feature_extractor.", "_masknet.")
  std::string prefix = "";
  // Whether conv() counts an identity K-segment (a residual added as it is) as 1 * 1 * cin MACs per
  // output. The networks differ and stay as they are, since flops_per_frame feeds the benchmark's
  // TFLOP/s: CenterpointDLA34 leaves its residuals out, ResNet-18 and the YOLACT head count them.
  bool identity_flops = true;

  std::string key(const std::string& n) const { return n.empty() ? n : prefix + n; }

  // ---------------- parameters, in state_dict order ----------------
  void add(const std::string& n, std::vector<int64_t> s) { P.params.push_back({prefix + n, std::move(s)}); }
  void conv_p(const std::string& p, int cout, int cin, int k, bool bias = true) {
    add(p + ".weight", {cout, cin, k, k});
    if (bias) add(p + ".bias", {cout});
  }
  void bn_p(const std::string& p, int c) {
    add(p + ".weight", {c});
    add(p + ".bias", {c});
    add(p + ".running_mean", {c});
    add(p + ".running_var", {c});
    add(p + ".num_batches_tracked", {});
  }

  // ---------------- tensors and K-segments ----------------
  int tensor(int H, int W, int C, bool f32 = false) {
    TensorSpec t{H, W, C};
    t.f32 = f32;
    P.tensors.push_back(t);
    return (int)P.tensors.size() - 1;
  }
  static int out_dim(int x, int k, int s, int pad) { return (x + 2 * pad - k) / s + 1; }
  static int pad4(int n) { return (n + 3) / 4 * 4; }  // an fp32 store writes whole 16-byte vectors
  // input channels [ci0, ci0 + cin) of the k x k Conv2d `w`, BatchNorm `bn` folded ("" = none)
  SegSpec seg(int src, const std::string& w, const std::string& bn, int ci0, int cin, int k, int stride, int pad) const {
    return SegSpec{src, key(w), key(bn), ci0, cin, k, k, stride, pad};
  }
  // the whole weight at "same" padding
  SegSpec seg(int src, const std::string& w, const std::string& bn, int cin, int k, int stride) const {
    return seg(src, w, bn, 0, cin, k, stride, k / 2);
  }
  // `src` added as it is (bn empty) or through an eval BatchNorm (scaled per channel, shift in the bias)
  SegSpec identity(int src, int c, const std::string& bn = "") const {
    SegSpec sg = seg(src, "", bn, 0, c, 1, 1, 0);
    sg.identity = true;
    return sg;
  }
  // a 7x7 / padding 3 stem over the row-expanded staged image (staged_image): a 7x1 conv there
  SegSpec stem7(int img, const std::string& w, const std::string& bn, int stride) const {
    SegSpec sg = seg(img, w, bn, 0, 3, 7, stride, 3);
    sg.kw = 1;
    sg.pad_w = 0;
    sg.row_expand = 7;
    return sg;
  }

  // ---------------- ops ----------------
  // a hand-filled op into the tensor, or the caller's output, that `op.out` names already
  int emit(OpSpec op) {
    op.label = prefix + op.label;
    P.ops.push_back(std::move(op));
    return P.ops.back().out;
  }
  // ... into a new [H, W, C] tensor
  int emit(OpSpec op, int H, int W, int C, bool f32 = false) {
    op.out = tensor(H, W, C, f32);
    return emit(std::move(op));
  }
  // one fused GEMM over the K-segments; the output size is segment 0's
  int conv(const std::string& label, std::vector<SegSpec> segs, int N, int act) {
    const SegSpec& s0 = segs[0];
    const int Ho = out_dim(P.tensors[s0.src].H, s0.kh, s0.stride, s0.pad);
    const int Wo = out_dim(P.tensors[s0.src].W, s0.kw, s0.stride, s0.pad_w >= 0 ? s0.pad_w : s0.pad);
    OpSpec op;
    op.kind = OP_CONV;
    op.label = label;
    op.N = N;
    op.act = act;
    for (const SegSpec& sg : segs)
      if (identity_flops || !sg.identity)
        op.flops += 2.0 * Ho * Wo * N * (double)(sg.kh * (sg.row_expand ? sg.row_expand : sg.kw) * sg.cin);
    op.segs = std::move(segs);
    return emit(std::move(op), Ho, Wo, N);
  }
  // The input frame staged row-expanded for a 7x7 stem: pixel (y, x) holds the 7 horizontal taps
  // x-3..x+3 of its 3 channels (21 values, zero-padded to a whole 16-byte chunk), so the stem is a
  // 7x1 conv with K = 7 * in_cpad instead of 49 taps of a padded pixel.
  int staged_image(const tv_model_desc& d, const std::string& label) {
    const int vec = 16 / dtype_size(d.compute_dtype);
    P.in_cpad = (7 * 3 + vec - 1) / vec * vec;
    OpSpec op;
    op.kind = OP_PREP;
    op.label = label;
    op.N = P.in_cpad;
    return emit(std::move(op), d.in_h, d.in_w, P.in_cpad);
  }
  // `src` into the caller's fp32 NHWC output `slot` through an identity 1x1 GEMM (exact: one
  // product per output, fp32 accumulation; no FLOPs counted); returns that output's spec
  IoSpec to_caller_f32(int src, int slot, const std::string& label) {
    const TensorSpec t = P.tensors[src];
    OpSpec op;
    op.kind = OP_CONV;
    op.label = label;
    op.segs = {identity(src, t.C)};
    op.N = t.C;
    op.out = -1 - slot;
    emit(std::move(op));
    return IoSpec{t.H, t.W, t.C, t.C};
  }
  // the 3x3 convs `names` (ns[j] output channels each) over `src` as one GEMM, their weights stacked
  // along N (zero rows from their sum up to N)
  int stacked_conv3x3(const std::string& label, int src, const std::vector<std::string>& names, const std::vector<int>& ns,
                      int N, int act, bool f32 = false) {
    const TensorSpec t = P.tensors[src];
    int n = 0;
    for (int v : ns) n += v;
    OpSpec op;
    op.kind = OP_CONV;
    op.label = label;
    op.segs = {seg(src, "", "", t.C, 3, 1)};
    for (const std::string& w : names) op.stack_w.push_back(key(w));
    op.stack_n = ns;
    op.N = N;
    op.act = act;
    op.out_f32 = f32;
    op.flops = 2.0 * t.H * t.W * n * 9.0 * t.C;
    return emit(std::move(op), t.H, t.W, N, f32);
  }
  // the 1x1 convs `names`, conv j from channels [hidden * j, + hidden) of `src` to ns[j] channels, as
  // one block-diagonal GEMM into the caller's fp32 NHWC output `slot`; returns that output's spec
  IoSpec block_diag_1x1(const std::string& label, int src, const std::vector<std::string>& names, const std::vector<int>& ns,
                        int hidden, int act, int slot) {
    const TensorSpec t = P.tensors[src];
    OpSpec op;
    op.kind = OP_CONV;
    op.label = label;
    op.segs = {seg(src, "", "", t.C, 1, 1)};
    int ctot = 0;
    for (size_t j = 0; j < names.size(); ++j) {
      op.stack_w.push_back(key(names[j]));
      op.stack_n.push_back(ns[j]);
      op.diag_in_off.push_back(hidden * (int)j);
      op.diag_out_off.push_back(ctot);
      op.flops += 2.0 * t.H * t.W * ns[j] * (double)hidden;
      ctot += ns[j];
    }
    op.N = pad4(ctot);
    op.act = act;
    op.out = -1 - slot;
    emit(std::move(op));
    return IoSpec{t.H, t.W, ctot, pad4(ctot)};
  }
  // CenterNet-style heads `<key><h>.0` (3x3 to `hidden` channels, activation `act`) and `<key><h>.2`
  // (1x1 to head_channels[h], fp32 output 0): the stacked GEMM, then the block-diagonal one
  IoSpec stacked_heads(int src, const std::string& key0, int n_heads, const int32_t* head_channels, int hidden, int act,
                       const std::string& label0, const std::string& label2) {
    std::vector<std::string> w0, w2;
    for (int h = 0; h < n_heads; ++h) {
      w0.push_back(key0 + std::to_string(h) + ".0");
      w2.push_back(key0 + std::to_string(h) + ".2");
    }
    const int mid = stacked_conv3x3(label0, src, w0, std::vector<int>(n_heads, hidden), hidden * n_heads, act);
    return block_diag_1x1(label2, mid, w2, std::vector<int>(head_channels, head_channels + n_heads), hidden, 0, 0);
  }
  // the single-output archs' output geometry
  void single_output(const IoSpec& o) { P.out_h = o.H, P.out_w = o.W, P.out_c = o.C, P.out_cpad = o.cpad; }

  // Once per plan, after the last op: the key set, the FLOPs (summed in op order) and the GEMMs'
  // K-segment limit (only a CenterNet Root over a tree of height 8 can pass it).
  int finish() {
    for (const ParamInfo& p : P.params) P.names.insert(p.name);
    for (const OpSpec& op : P.ops) P.flops_per_frame += op.flops;
    for (const OpSpec& op : P.ops)
      if (op.kind == OP_CONV && op.segs.size() > (size_t)kMaxSeg) {
        set_error("too many concatenated inputs for one Root (tree height too large)");
        return TV_ESHAPE;
      }
    return TV_OK;
  }
};

}  // namespace tv
