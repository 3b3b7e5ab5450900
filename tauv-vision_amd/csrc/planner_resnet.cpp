// Planner for the YOLACT backbone, reference Resnet101Backbone (src/tauv_vision/yolact/model/
// backbone.py:9-32): despite its name torchvision's resnet18, tapped at layer2.1.bn2, layer3.1.bn2
// and layer4.1.bn2 by create_feature_extractor.
//  (1) parameter registration order = torchvision ResNet(BasicBlock, [2, 2, 2, 2]).state_dict()
//      without fc: `conv1`, `bn1`, then per layer L = 1..4 and block B = 0, 1 `layerL.B.conv1`,
//      `.bn1`, `.conv2`, `.bn2` and, for the first block of layers 2..4, `.downsample.0` (1x1 conv,
//      stride 2) and `.downsample.1` (BatchNorm); every conv bias-free. torchvision is not available
//      to this project's tests, so these names are restated, not pinned: the assumption
//      is that the feature extractor's GraphModule keeps the qualified names and drops `fc`.
//  (2) the forward pass lowered over NHWC tensors:
//        * conv1 7x7 / s2 / p3 + bn1 + ReLU      -> one GEMM over the row-expanded staged image
//        * MaxPool2d(3, 2, 1)                     -> OP_MAXPOOL3S2
//        * BasicBlock: relu(bn1(conv1(x))), then relu(bn2(conv2(h)) + residual) -> two GEMMs, the
//          second with the residual as a K-segment: the identity, or the block's folded 1x1 / s2
//          `downsample`
//        * the tapped blocks layer2.1 and layer3.1: conv2 stores bn2(conv2(h)) with no activation —
//          the tap, which is the output of bn2, before the add and the ReLU — and OP_ADD_RELU forms
//          relu(tap + x) for the next layer; layer4.1 ends at its tap (its add and ReLU feed nothing)
#include "plan_builder.h"

namespace tv {
namespace {

struct ResnetWalker : PlanBuilder {  // `prefix` in front of every key and label
  void params() {  // every conv bias-free
    conv_p("conv1", 64, 3, 7, false);
    bn_p("bn1", 64);
    int cin = 64;
    for (int L = 1; L <= 4; ++L) {
      const int c = 64 << (L - 1);
      for (int b = 0; b < 2; ++b) {
        const std::string p = "layer" + std::to_string(L) + "." + std::to_string(b);
        conv_p(p + ".conv1", c, b ? c : cin, 3, false);
        bn_p(p + ".bn1", c);
        conv_p(p + ".conv2", c, c, 3, false);
        bn_p(p + ".bn2", c);
        if (!b && L > 1) {
          conv_p(p + ".downsample.0", c, cin, 1, false);
          bn_p(p + ".downsample.1", c);
        }
      }
      cin = c;
    }
  }

  // an elementwise (stride 1) or 3x3 / padding 1 window (stride 2, floor mode) op over `src`
  int elementwise(int kind, const std::string& label, int src, int add, int stride) {
    const TensorSpec t = P.tensors[src];
    OpSpec op;
    op.kind = kind;
    op.label = label;
    op.src = src;
    op.add = add;
    op.N = t.C;
    return emit(op, out_dim(t.H, 3, stride, 1), out_dim(t.W, 3, stride, 1), t.C);
  }

  std::vector<int> forward(int img) {
    int x = conv("conv1 + bn1 + ReLU", {stem7(img, "conv1", "bn1", 2)}, 64, 1);
    x = elementwise(OP_MAXPOOL3S2, "maxpool", x, -1, 2);
    std::vector<int> taps;
    int cin = 64;
    for (int L = 1; L <= 4; ++L) {
      const int c = 64 << (L - 1);
      for (int b = 0; b < 2; ++b) {
        const std::string p = "layer" + std::to_string(L) + "." + std::to_string(b);
        const int stride = !b && L > 1 ? 2 : 1;
        const int h = conv(p + ".conv1 + bn1 + ReLU", {seg(x, p + ".conv1", p + ".bn1", b ? c : cin, 3, stride)}, c, 1);
        const SegSpec c2 = seg(h, p + ".conv2", p + ".bn2", c, 3, 1);
        if (b && L > 1) {  // a tapped block
          const int tap = conv(p + ".conv2 + bn2 (tap)", {c2}, c, 0);
          taps.push_back(tap);
          if (L < 4) x = elementwise(OP_ADD_RELU, p + " relu(bn2 + x)", tap, x, 1);
        } else if (stride == 2) {
          x = conv(p + ".conv2 + bn2 + downsample + ReLU", {c2, seg(x, p + ".downsample.0", p + ".downsample.1", cin, 1, 2)},
                   c, 1);
        } else {
          x = conv(p + ".conv2 + bn2 + x + ReLU", {c2, identity(x, c)}, c, 1);
        }
      }
      cin = c;
    }
    return taps;
  }
};

}  // namespace

std::vector<int> append_resnet18(Plan& P, const std::string& prefix, int img) {
  ResnetWalker w{{P, prefix}};
  w.params();
  return w.forward(img);
}

int build_plan_resnet(const tv_model_desc& d, Plan* plan) {
  if (d.in_h < 1 || d.in_w < 1 || d.compute_dtype < 0 || d.compute_dtype > 2) {
    set_error("resnet18 desc: need in_h, in_w >= 1 and a compute dtype");
    return TV_EINVAL;
  }
  // the head's desc over the taps, checked before anything is planned: depths fixed, sizes by the conv arithmetic
  tv_model_desc hd = d;
  if (d.arch == TV_ARCH_YOLACT) {
    hd.n_levels = hd.n_maps = 3;
    int h = d.in_h, w = d.in_w;
    for (int i = 0; i < 2; ++i) h = (h - 1) / 2 + 1, w = (w - 1) / 2 + 1;
    for (int i = 0; i < 3; ++i) {
      h = (h - 1) / 2 + 1, w = (w - 1) / 2 + 1;
      hd.channels[1 + i] = 128 << i;
      hd.map_h[i] = h;
      hd.map_w[i] = w;
    }
    for (int i = 4; i < 9; ++i) hd.channels[i] = 0;
    const int rc = check_yolact_head_desc(hd);
    if (rc) return rc;
  }
  *plan = Plan();
  Plan& P = *plan;
  PlanBuilder b{P};
  const int img = b.staged_image(d, "input staging (NCHW fp32 -> NHWC)");
  P.in_channels = 3;
  P.ins.push_back(IoSpec{d.in_h, d.in_w, 3, 3});
  const std::vector<int> taps = append_resnet18(P, d.arch == TV_ARCH_YOLACT ? "_backbone._feature_extractor." : "", img);
  if (d.arch == TV_ARCH_YOLACT) {
    append_yolact_head(P, hd, taps);
  } else {
    for (size_t i = 0; i < taps.size(); ++i) {  // the taps also feed the next layer's add: copied out of the arena
      const TensorSpec t = P.tensors[taps[i]];
      OpSpec o;
      o.kind = OP_STORE_F32;
      o.label = "layer" + std::to_string(i + 2) + ".1.bn2 -> fp32 NHWC";
      o.src = taps[i];
      o.N = t.C;
      o.out = -1 - (int)i;
      P.outs.push_back(IoSpec{t.H, t.W, t.C, t.C});
      b.emit(o);
    }
  }
  return TV_OK;
}

}  // namespace tv
