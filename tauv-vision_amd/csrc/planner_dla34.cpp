// Planner for the reference's CenterpointDLA34 (src/tauv_vision/centernet/model/backbones/
// centerpoint_dla.py): the module tree walked twice, like planner.cpp does for Centernet —
//  (1) parameter registration order = the reference state_dict layout (keys `model.*`,
//      CenterpointDLA34 wraps DLASeg as `self.model`, :549-556), so checkpoints load by key;
//  (2) the forward pass (:30-59, 147-221, 224-306, 360-462, 476-525) lowered to fused GEMMs and
//      bandwidth kernels over NHWC tensors:
//        * conv(bias=False) + BN + ReLU                 -> one GEMM, BN folded
//        * BasicBlock conv2 + residual (+= , ReLU)      -> one GEMM; the residual is a second
//          K-segment: Tree.project's 1x1 + BN over the max-pooled bottom, or an identity 1x1
//        * Root 1x1 over torch.cat(children)            -> one GEMM, one K-segment per child
//        * Tree.downsample MaxPool2d(2, 2, ceil_mode)   -> OP_MAXPOOL
//        * DeformConv: offset + mask 3x3 convs          -> one GEMM (N = 18 + 9, padded to 32)
//                      DCNv2 bilinear sampling x mask   -> OP_DCN (9-tap column tensor)
//                      DeformConv2d + bias + BN + ReLU  -> one GEMM over the columns (K = 9 * C)
//        * IDAUp depthwise ConvTranspose2d + pad_to_match + add -> OP_DWCONVT_ADD
//        * heads: 3x3 (64 -> 256) + bias + ReLU, stacked -> one GEMM (N = 256 * heads);
//                 1x1 (256 -> n) + bias -> one block-diagonal GEMM into the fp32 output
// The outer Tree's `project` of a height-2 tree is computed by the reference but never read
// (its tree1 recomputes its own residual, :209-216): it is not lowered.
#include <algorithm>
#include <map>

#include "plan_builder.h"

namespace tv {
namespace {

constexpr int kLevels[6] = {1, 1, 1, 2, 2, 1};       // dla34(), :309-315
constexpr int kChannels[6] = {16, 32, 64, 128, 256, 512};
constexpr int kHeadConv = 256;                       // get_pose_net head_conv, :534-541
constexpr int kFirstLevel = 2, kLastLevel = 5;       // down_ratio 4, last_level 5

struct DlaWalker : PlanBuilder {
  const tv_model_desc& d;
  std::map<int, int> pooled;  // tensor -> its max-pooled tensor (shared by tree1 and the Root)
  // identity_flops off: a BasicBlock's residual added as it is counts no FLOPs in this network
  DlaWalker(const tv_model_desc& desc, Plan& plan) : PlanBuilder{plan, "", false}, d(desc) {}

  // ---------------- (1) parameters ----------------
  void conv_w(const std::string& p, int cout, int cin, int k) { conv_p(p, cout, cin, k, false); }  // bias=False
  void conv_wb(const std::string& p, int cout, int cin, int k) { conv_p(p, cout, cin, k); }
  void basic_p(const std::string& p, int cin, int cout) {
    conv_w(p + ".conv1", cout, cin, 3);
    bn_p(p + ".bn1", cout);
    conv_w(p + ".conv2", cout, cout, 3);
    bn_p(p + ".bn2", cout);
  }
  // Tree.__init__ (:168-200): tree1, tree2, [root], [project]
  void tree_p(const std::string& p, int levels, int cin, int cout, bool level_root, int root_dim) {
    if (root_dim == 0) root_dim = 2 * cout;
    if (level_root) root_dim += cin;
    if (levels == 1) {
      basic_p(p + ".tree1", cin, cout);
      basic_p(p + ".tree2", cout, cout);
    } else {
      tree_p(p + ".tree1", levels - 1, cin, cout, false, 0);
      tree_p(p + ".tree2", levels - 1, cout, cout, false, root_dim + cout);
    }
    if (levels == 1) {
      conv_w(p + ".root.conv", cout, root_dim, 1);
      bn_p(p + ".root.bn", cout);
    }
    if (cin != cout) {
      conv_w(p + ".project.0", cout, cin, 1);
      bn_p(p + ".project.1", cout);
    }
  }
  void deform_p(const std::string& p, int chi, int cho) {  // DeformConv (:360-384)
    bn_p(p + ".actf.0", cho);
    conv_wb(p + ".offset", 18, chi, 3);
    conv_wb(p + ".mask", 9, chi, 3);
    conv_wb(p + ".conv", cho, chi, 3);
  }
  // IDAUp.__init__ (:411-428): per i: proj_i, up_i, node_i
  void ida_p(const std::string& p, int o, const std::vector<int>& ch, const std::vector<int>& up_f) {
    for (size_t i = 1; i < ch.size(); ++i) {
      const int f = up_f[i];
      deform_p(p + ".proj_" + std::to_string(i), ch[i], o);
      add(p + ".up_" + std::to_string(i) + ".weight", {o, 1, 2 * f, 2 * f});
      deform_p(p + ".node_" + std::to_string(i), o, o);
    }
  }
  // DLAUp.__init__ (:435-449): the IDAUps and their channel / scale bookkeeping (in_channels
  // aliases `channels` and is rewritten as the loop goes)
  struct IdaDef { int o; std::vector<int> ch, up_f; };
  std::vector<IdaDef> dla_up_defs() const {
    std::vector<int> channels(kChannels + kFirstLevel, kChannels + 6), in_ch = channels;
    std::vector<int> scales;
    for (size_t i = 0; i < channels.size(); ++i) scales.push_back(1 << i);
    std::vector<IdaDef> defs;
    const int n = (int)channels.size();
    for (int i = 0; i < n - 1; ++i) {
      const int j = n - i - 2;
      IdaDef def{channels[j], std::vector<int>(in_ch.begin() + j, in_ch.end()), {}};
      for (int k = j; k < n; ++k) def.up_f.push_back(scales[k] / scales[j]);
      defs.push_back(def);
      for (int k = j + 1; k < n; ++k) {
        scales[k] = scales[j];
        in_ch[k] = channels[j];
      }
    }
    return defs;
  }
  IdaDef ida_up_def() const {  // DLASeg.ida_up (:491-492)
    IdaDef def{kChannels[kFirstLevel], {}, {}};
    for (int l = kFirstLevel; l < kLastLevel; ++l) {
      def.ch.push_back(kChannels[l]);
      def.up_f.push_back(1 << (l - kFirstLevel));
    }
    return def;
  }
  void params() {
    const std::string b = "model.base";
    conv_w(b + ".base_layer.0", kChannels[0], 3, 7);
    bn_p(b + ".base_layer.1", kChannels[0]);
    int cin = kChannels[0];
    for (int l = 0; l < 2; ++l)
      for (int c = 0; c < kLevels[l]; ++c) {
        conv_w(b + ".level" + std::to_string(l) + "." + std::to_string(3 * c), kChannels[l], cin, 3);
        bn_p(b + ".level" + std::to_string(l) + "." + std::to_string(3 * c + 1), kChannels[l]);
        cin = kChannels[l];
      }
    for (int l = 2; l < 6; ++l)
      tree_p(b + ".level" + std::to_string(l), kLevels[l], kChannels[l - 1], kChannels[l], l >= 3, 0);
    const auto defs = dla_up_defs();
    for (size_t i = 0; i < defs.size(); ++i) ida_p("model.dla_up.ida_" + std::to_string(i), defs[i].o, defs[i].ch, defs[i].up_f);
    const IdaDef iu = ida_up_def();
    ida_p("model.ida_up", iu.o, iu.ch, iu.up_f);
    for (int h = 0; h < d.n_heads; ++h) {
      conv_wb("model." + std::to_string(h) + ".0", kHeadConv, kChannels[kFirstLevel], 3);
      conv_wb("model." + std::to_string(h) + ".2", d.head_channels[h], kHeadConv, 1);
    }
  }

  // ---------------- (2) forward lowering ----------------
  int maxpool(int x) {
    auto it = pooled.find(x);
    if (it != pooled.end()) return it->second;
    const TensorSpec t = P.tensors[x];
    OpSpec op;
    op.kind = OP_MAXPOOL;
    op.label = "MaxPool2d(2, 2, ceil_mode=True)";
    op.src = x;
    op.N = t.C;
    return pooled[x] = emit(op, (t.H + 1) / 2, (t.W + 1) / 2, t.C);
  }
  // BasicBlock (:30-59) with its residual as the second K-segment of conv2
  int basic(const std::string& p, int x, int cin, int cout, int stride, SegSpec res) {
    int t = conv(p + ".conv1", {seg(x, p + ".conv1", p + ".bn1", 0, cin, 3, stride, 1)}, cout, 1);
    const TensorSpec to = P.tensors[t], tr = P.tensors[res.src];
    if (tr.H != to.H || tr.W != to.W) {  // pad_to_match never fires for stride-2 ceil pooling
      set_error("DLA34 BasicBlock residual shape mismatch");
      return -1;
    }
    return conv(p + ".conv2+residual", {seg(t, p + ".conv2", p + ".bn2", 0, cout, 3, 1, 1), res}, cout, 1);
  }
  int root(const std::string& p, const std::vector<int>& kids, int cout) {
    std::vector<SegSpec> segs;
    int off = 0;
    for (int k : kids) {
      const int c = P.tensors[k].C;
      segs.push_back(seg(k, p + ".conv", p + ".bn", off, c, 1, 1, 0));
      off += c;
    }
    return conv(p + ".conv", segs, cout, 1);
  }
  // Tree.forward (:202-221)
  int tree(const std::string& p, int x, int levels, int stride, int cin, int cout, bool level_root,
           std::vector<int> children) {
    const int bottom = stride > 1 ? maxpool(x) : x;
    if (level_root) children.push_back(bottom);
    if (levels == 1) {
      const SegSpec res = cin != cout ? seg(bottom, p + ".project.0", p + ".project.1", 0, cin, 1, 1, 0)
                                      : identity(bottom, cin);
      const int x1 = basic(p + ".tree1", x, cin, cout, stride, res);
      if (x1 < 0) return -1;
      const int x2 = basic(p + ".tree2", x1, cout, cout, 1, identity(x1, cout));
      if (x2 < 0) return -1;
      std::vector<int> kids{x2, x1};
      kids.insert(kids.end(), children.begin(), children.end());
      return root(p + ".root", kids, cout);
    }
    const int x1 = tree(p + ".tree1", x, levels - 1, stride, cin, cout, false, {});
    if (x1 < 0) return -1;
    children.push_back(x1);
    return tree(p + ".tree2", x1, levels - 1, 1, cout, cout, false, children);
  }
  // DeformConv.forward (:386-392)
  int deform(const std::string& p, int x, int cho) {
    const TensorSpec t = P.tensors[x];
    OpSpec dc;
    dc.kind = OP_DCN;
    dc.label = p + ".conv (DCNv2 sampling)";
    dc.src = x;
    // N = 32: 18 offsets (dy, dx per tap) + 9 mask logits + 5 zero columns
    dc.add = stacked_conv3x3(p + ".offset+mask", x, {p + ".offset", p + ".mask"}, {18, 9}, 32, 0);
    dc.N = 9 * t.C;
    SegSpec cs = seg(emit(dc, t.H, t.W, 9 * t.C), p + ".conv", p + ".actf.0", 0, t.C, 1, 1, 0);
    cs.row_expand = 9;
    return conv(p + ".conv+actf", {cs}, cho, 1);
  }
  // IDAUp.forward (:453-460): layers[i] = node(pad_to_match(up(proj(layers[i]))) + layers[i-1])
  int ida(const std::string& p, std::vector<int>& layers, int startp, int endp, int o) {
    for (int i = startp + 1; i < endp; ++i) {
      const std::string js = std::to_string(i - startp);
      const int pr = deform(p + ".proj_" + js, layers[i], o);
      const TensorSpec src = P.tensors[pr], tgt = P.tensors[layers[i - 1]];
      const std::string uw = p + ".up_" + js;
      int f = 0;
      for (const ParamInfo& pi : P.params)
        if (pi.name == uw + ".weight") f = (int)pi.shape[2] / 2;
      if (f < 1) {
        set_error("DLA34 planner: missing " + uw);
        return -1;
      }
      const int hu = (src.H - 1) * f - 2 * (f / 2) + 2 * f, wu = (src.W - 1) * f - 2 * (f / 2) + 2 * f;
      OpSpec op;
      op.kind = OP_DWCONVT_ADD;
      op.label = uw + "+pad_to_match+add";
      op.src = pr;
      op.add = layers[i - 1];
      op.up_s = f;
      op.up_w = uw;
      op.N = o;
      op.sy = std::max(0, (hu - tgt.H) / 2);  // pad_to_match (:394-407), (W, H) order correct here
      op.sx = std::max(0, (wu - tgt.W) / 2);
      op.flops = 2.0 * src.H * src.W * o * 4.0 * f * f;
      layers[i] = deform(p + ".node_" + js, emit(op, tgt.H, tgt.W, o), o);
    }
    return 0;
  }
  int forward() {
    const int img = staged_image(d, "input staging (NCHW fp32 / u8 frames -> NHWC)");
    const std::string b = "model.base";
    int x = conv(b + ".base_layer.0", {stem7(img, b + ".base_layer.0", b + ".base_layer.1", 1)}, kChannels[0], 1);
    std::vector<int> layers;
    int cin = kChannels[0];
    for (int l = 0; l < 2; ++l) {  // _make_conv_level (:288-297)
      for (int c = 0; c < kLevels[l]; ++c) {
        const std::string q = b + ".level" + std::to_string(l) + ".";
        x = conv(q + std::to_string(3 * c), {seg(x, q + std::to_string(3 * c), q + std::to_string(3 * c + 1), 0, cin, 3,
                                                 c == 0 ? (l == 1 ? 2 : 1) : 1, 1)},
                 kChannels[l], 1);
        cin = kChannels[l];
      }
      layers.push_back(x);
    }
    for (int l = 2; l < 6; ++l) {
      x = tree(b + ".level" + std::to_string(l), x, kLevels[l], 2, kChannels[l - 1], kChannels[l], l >= 3, {});
      if (x < 0) return TV_ESHAPE;
      layers.push_back(x);
    }
    // DLAUp.forward (:451-457)
    const auto defs = dla_up_defs();
    std::vector<int> out{layers.back()};
    const int n = (int)layers.size();
    for (int i = 0; i < n - kFirstLevel - 1; ++i) {
      if (ida("model.dla_up.ida_" + std::to_string(i), layers, n - i - 2, n, defs[i].o)) return TV_ESHAPE;
      out.insert(out.begin(), layers.back());
    }
    // DLASeg.forward (:515-525)
    std::vector<int> y(out.begin(), out.begin() + (kLastLevel - kFirstLevel));
    if (ida("model.ida_up", y, 0, (int)y.size(), ida_up_def().o)) return TV_ESHAPE;
    single_output(stacked_heads(y.back(), "model.", d.n_heads, d.head_channels, kHeadConv, 1,
                                "model.*.0 (stacked heads) + ReLU", "model.*.2 (block-diagonal) -> fp32 NHWC"));
    return 0;
  }
};

}  // namespace

int build_plan_dla34(const tv_model_desc& d, Plan* plan) {
  if (d.n_heads < 1 || d.n_heads > 16 || d.in_h < 1 || d.in_w < 1 || d.compute_dtype < 0 || d.compute_dtype > 2) {
    set_error("model desc out of range");
    return TV_EINVAL;
  }
  for (int h = 0; h < d.n_heads; ++h)
    if (d.head_channels[h] < 1) {
      set_error("head channel counts must be positive");
      return TV_EINVAL;
    }
  if (d.in_h < 32 || d.in_w < 32) {
    set_error("CenterpointDLA34 needs frames of at least 32x32 (five stride-2 levels)");
    return TV_ESHAPE;
  }
  *plan = Plan();
  DlaWalker w(d, *plan);
  w.params();
  return w.forward();
}

}  // namespace tv
