// Planner for everything of the reference Yolact.forward after the backbone (model.py:34-60):
// FeaturePyramid (feature_pyramid.py:8-58), the one PredictionHead shared by every level
// (prediction_head.py:9-143) and Masknet on fpn[0] (planner_protonet.cpp), and for the
// FeaturePyramid alone (TV_ARCH_YOLACT_FPN).
//  (1) parameter registration order = Yolact.state_dict() without `_backbone.*` (model.py:25-29):
//      `_feature_pyramid.` {`_lateral_layers.i`, `_downsample_layers.i`, `_prediction_layers.i`},
//      `_masknet.*`, `_prediction_head.` {per group trunk / classification / box / mask:
//      `_X_layers.i` (torchvision Bottleneck: conv1, bn1, conv2, bn2, conv3, bn3, bias-free convs),
//      `_X_conv_layers.i`, `_X_bn_layers.i`; then `_classification_layer`, `_box_encoding_layer`,
//      `_mask_coeff_layer`};
//  (2) the forward pass lowered over NHWC tensors:
//        * backbone map i fp32 NCHW -> NHWC compute dtype       -> OP_LAYOUT_IN (input i)
//        * lateral 1x1 convs                                    -> one GEMM each
//        * p_i = lateral_i + bilinear(p_{i+1})                  -> OP_BILINEAR_ADD, in place
//        * 3x3 (+ stride-2 3x3 for the extra levels) + LeakyReLU -> one GEMM each
//        * per level, x = relu(conv1x1(x) + BN(Bottleneck(x))) -> four GEMMs: the Bottleneck's three
//          convs (BN folded, its residual an identity K-segment), then the 1x1 conv with the
//          Bottleneck output as a second K-segment: the outer BatchNorm follows a ReLU, so it cannot
//          fold into a conv — it is an identity segment scaled per channel, its shift in the bias
//        * the three final 3x3 convs -> fp32 raw tensors in the arena (the GEMMs' fp32 store: the
//          logits and box regressions are never rounded to the compute dtype); one GEMM with the
//          weights stacked along N when no branch has blocks of its own
//        * raw tensors -> the caller's [A_total, width] outputs -> OP_HEAD_SCATTER per level
// Two reference quirks are kept: one PredictionHead for all levels (each level's ops read the same
// weights), and the pixel-major, aspect-ratio-inner row order of permute(0, 2, 3, 1).reshape
// (prediction_head.py:112-113), which differs from get_anchor's ratio-major blocks (anchors.py).
#include "plan_builder.h"

namespace tv {
namespace {

struct HeadWalker : PlanBuilder {
  const tv_model_desc& d;
  const int F;
  const bool head;
  const std::vector<int>& given;  // the backbone maps when they are tensors of the plan already (else empty)

  void fpn_params(const std::string& p) {
    for (int i = 0; i < d.n_levels; ++i) conv_p(p + "_lateral_layers." + std::to_string(i), F, d.channels[1 + i], 1);
    for (int i = 0; i < d.downsamples; ++i) conv_p(p + "_downsample_layers." + std::to_string(i), F, F, 3);
    for (int i = 0; i < d.n_levels; ++i) conv_p(p + "_prediction_layers." + std::to_string(i), F, F, 3);
  }
  void group_params(const std::string& p, const std::string& g, int n) {
    for (int i = 0; i < n; ++i) {
      const std::string b = p + g + "_layers." + std::to_string(i);
      conv_p(b + ".conv1", F / 4, F, 1, false);
      bn_p(b + ".bn1", F / 4);
      conv_p(b + ".conv2", F / 4, F / 4, 3, false);
      bn_p(b + ".bn2", F / 4);
      conv_p(b + ".conv3", F, F / 4, 1, false);
      bn_p(b + ".bn3", F);
    }
    for (int i = 0; i < n; ++i) conv_p(p + g + "_conv_layers." + std::to_string(i), F, F, 1);
    for (int i = 0; i < n; ++i) bn_p(p + g + "_bn_layers." + std::to_string(i), F);
  }

  // backbone map i, one of the caller's inputs, as an NHWC tensor
  int layout_in(int i) {
    const int c = d.channels[1 + i];
    P.ins.push_back(IoSpec{d.map_h[i], d.map_w[i], c, c});
    OpSpec op;
    op.kind = OP_LAYOUT_IN;
    op.label = "backbone map " + std::to_string(i) + " NCHW fp32 -> NHWC";
    op.N = c;
    op.io = i;
    return emit(op, d.map_h[i], d.map_w[i], c);
  }

  // feature_pyramid.py:44-58 -> the FPN levels' tensors
  std::vector<int> fpn(const std::string& p) {
    const int n = d.n_levels;
    std::vector<int> lat(n);
    for (int i = 0; i < n; ++i) {
      const int c = d.channels[1 + i];
      const int x = given.empty() ? layout_in(i) : given[i];
      const std::string w = p + "_lateral_layers." + std::to_string(i);
      lat[i] = conv(w, {seg(x, w, "", c, 1, 1)}, F, 0);
    }
    for (int i = n - 2; i >= 0; --i) {
      OpSpec op;
      op.kind = OP_BILINEAR_ADD;
      op.label = "pyramid " + std::to_string(i) + " = lateral + bilinear(pyramid " + std::to_string(i + 1) + ")";
      op.src = lat[i + 1];
      op.add = lat[i];
      op.out = lat[i];
      op.N = F;
      emit(op);
    }
    std::vector<int> lv;
    for (int i = 0; i < n; ++i) {
      const std::string w = p + "_prediction_layers." + std::to_string(i);
      lv.push_back(conv(w + " + LeakyReLU", {seg(lat[i], w, "", F, 3, 1)}, F, 2));
    }
    for (int i = 0; i < d.downsamples; ++i) {
      const std::string w = p + "_downsample_layers." + std::to_string(i);
      lv.push_back(conv(w + " + LeakyReLU", {seg(lv.back(), w, "", F, 3, 2)}, F, 2));
    }
    return lv;
  }

  // x = relu(conv(x) + bn(bottleneck(x))) (prediction_head.py:93-98), n times
  int blocks(const std::string& lp, const std::string& p, const std::string& g, int n, int x) {
    for (int i = 0; i < n; ++i) {
      const std::string is = std::to_string(i);
      const std::string b = p + g + "_layers." + is;
      const int t1 = conv(lp + b + ".conv1", {seg(x, b + ".conv1", b + ".bn1", F, 1, 1)}, F / 4, 1);
      const int t2 = conv(lp + b + ".conv2", {seg(t1, b + ".conv2", b + ".bn2", F / 4, 3, 1)}, F / 4, 1);
      const int y = conv(lp + b + ".conv3 + x", {seg(t2, b + ".conv3", b + ".bn3", F / 4, 1, 1), identity(x, F, "")}, F, 1);
      const std::string c = p + g + "_conv_layers." + is;
      x = conv(lp + c + " + " + g + "_bn_layers." + is + "(bottleneck)",
               {seg(x, c, "", F, 1, 1), identity(y, F, p + g + "_bn_layers." + is)}, F, 1);
    }
    return x;
  }

  // a final 3x3 conv (or the three stacked along N) into an fp32 raw tensor
  int final_conv(const std::string& label, int x, const std::vector<std::string>& names, const std::vector<int>& ns) {
    int n = 0;
    for (int v : ns) n += v;
    return stacked_conv3x3(label, x, names, ns, pad4(n), 0, true);
  }

  void run() {
    const std::string fp = head ? "_feature_pyramid." : "";
    fpn_params(fp);
    const std::vector<int> lv = fpn(fp);
    if (!head) {
      for (size_t l = 0; l < lv.size(); ++l)  // each level into the caller's fp32 NHWC buffer
        P.outs.push_back(to_caller_f32(lv[l], (int)l, "fpn[" + std::to_string(l) + "] -> fp32 NHWC"));
      return;
    }
    const int k = d.head_channels[0], C1 = d.head_channels[1] + 1, nar = d.n_aspect_ratios;
    int A = 0;
    for (int t : lv) A += P.tensors[t].H * P.tensors[t].W * nar;
    P.outs = {IoSpec{A, 1, C1, C1}, IoSpec{A, 1, 4, 4}, IoSpec{A, 1, k, k}, IoSpec{}};
    P.outs[3] = append_protonet(P, "_masknet.", lv[0], F, k, 3);
    const std::string hp = "_prediction_head.";
    group_params(hp, "_extra", d.heights[0]);
    group_params(hp, "_classification_extra", d.heights[1]);
    group_params(hp, "_box_extra", d.heights[2]);
    group_params(hp, "_mask_extra", d.heights[3]);
    const std::vector<std::string> fin{hp + "_classification_layer", hp + "_box_encoding_layer", hp + "_mask_coeff_layer"};
    const std::vector<int> width{C1, 4, k};
    for (int j = 0; j < 3; ++j) conv_p(fin[j], nar * width[j], F, 3);
    const bool stacked = !d.heights[1] && !d.heights[2] && !d.heights[3];
    int row0 = 0;
    for (size_t l = 0; l < lv.size(); ++l) {
      const std::string lp = "level " + std::to_string(l) + " ";
      const TensorSpec t = P.tensors[lv[l]];
      const int x = blocks(lp, hp, "_extra", d.heights[0], lv[l]);
      OpSpec sc;
      sc.kind = OP_HEAD_SCATTER;
      sc.label = lp + "raw heads -> classification / box_encoding / tanh(mask_coeff)";
      if (stacked) {
        const int raw = final_conv(lp + "final 3x3 convs (stacked)", x, fin, {nar * C1, nar * 4, nar * k});
        int c0 = 0;
        for (int j = 0; j < 3; ++j) {
          sc.parts.push_back(ScatterPart{raw, c0, nar * width[j], j, row0, width[j], j == 2});
          c0 += nar * width[j];
        }
      } else {
        const char* g[3] = {"_classification_extra", "_box_extra", "_mask_extra"};
        for (int j = 0; j < 3; ++j) {
          const int xb = blocks(lp, hp, g[j], d.heights[1 + j], x);
          const int raw = final_conv(lp + fin[j], xb, {fin[j]}, {nar * width[j]});
          sc.parts.push_back(ScatterPart{raw, 0, nar * width[j], j, row0, width[j], j == 2});
        }
      }
      emit(sc);
      row0 += t.H * t.W * nar;
    }
  }
};

}  // namespace

int check_yolact_head_desc(const tv_model_desc& d) {
  const bool head = d.arch != TV_ARCH_YOLACT_FPN;
  if (d.compute_dtype < 0 || d.compute_dtype > 2 || d.n_levels < 1 || d.downsamples < 0 ||
      d.n_levels + d.downsamples > kMaxIO) {
    set_error("yolact head desc: need 1..8 backbone maps and FPN levels in all");
    return TV_EINVAL;
  }
  if (d.n_maps != d.n_levels) {
    set_error("yolact head desc: " + std::to_string(d.n_maps) + " map sizes for " + std::to_string(d.n_levels) +
              " backbone maps");
    return TV_EINVAL;
  }
  const int vec = 16 / dtype_size(d.compute_dtype);
  const int F = d.channels[0];
  for (int i = 0; i <= d.n_levels; ++i)
    if (d.channels[i] < 1 || d.channels[i] % vec) {
      set_error("yolact head desc: feature_depth and the backbone depths must be multiples of " + std::to_string(vec) +
                " for this dtype");
      return TV_ESHAPE;
    }
  for (int i = 0; i < d.n_levels; ++i)
    if (d.map_h[i] < 1 || d.map_w[i] < 1) {
      set_error("yolact head desc: map sizes must be positive");
      return TV_EINVAL;
    }
  if (head) {
    if (d.n_aspect_ratios < 1) {
      set_error("yolact head desc: need at least one anchor aspect ratio");
      return TV_EINVAL;
    }
    bool any = false, ok = d.n_heads == 2 && d.head_channels[0] >= 1 && d.head_channels[1] >= 1;
    for (int j = 0; j < 4; ++j) {
      ok = ok && d.heights[j] >= 0 && d.heights[j] <= 8;
      any = any || d.heights[j] > 0;
    }
    if (!ok) {
      set_error("yolact head desc: need head_channels = (n_prototype_masks, n_classes) and four layer counts in 0..8");
      return TV_EINVAL;
    }
    if (any && (F % 4 || (F / 4) % vec)) {
      set_error("yolact head desc: the Bottleneck width feature_depth / 4 must be a multiple of " + std::to_string(vec) +
                " for this dtype");
      return TV_ESHAPE;
    }
  }
  return TV_OK;
}

void append_yolact_head(Plan& P, const tv_model_desc& d, const std::vector<int>& maps) {
  HeadWalker w{{P}, d, d.channels[0], d.arch != TV_ARCH_YOLACT_FPN, maps};
  w.run();
}

int build_plan_yolact_head(const tv_model_desc& d, Plan* plan) {
  const int rc = check_yolact_head_desc(d);
  if (rc) return rc;
  *plan = Plan();
  append_yolact_head(*plan, d, {});
  plan->in_channels = d.channels[1];
  return TV_OK;
}

}  // namespace tv
