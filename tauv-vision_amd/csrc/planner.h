// The network planners' common output, a Plan: the reference state_dict layout of a model desc
// (parameters in registration order) and its forward pass lowered to a list of ops over NHWC
// tensors, fused GEMMs for the most part. One planner per network: the "R18" CenterNet (planner.cpp),
// CenterpointDLA34 (planner_dla34.cpp), and YOLACT's ResNet-18 backbone, neck + head and protonet
// (planner_resnet.cpp, planner_yolact_head.cpp, planner_protonet.cpp); all of them build their plan
// with plan_builder.h.
#pragma once
#include <cstdint>
#include <set>
#include <string>
#include <vector>

#include "../../include/tauv_vision_amd.h"

namespace tv {

struct ParamInfo {
  std::string name;
  std::vector<int64_t> shape;
};

// One K-segment of a fused conv: input channels [ci0, ci0 + cin) of a PyTorch conv weight,
// applied to tensor `src` (whose stored channel count may be padded beyond cin).
struct SegSpec {
  int src;               // tensor id
  std::string wname;     // "<prefix>.weight" of the Conv2d
  std::string bn;        // BatchNorm2d prefix folded into this conv ("" = none)
  int ci0, cin;          // slice of the weight's input channels
  int kh, kw, stride, pad;
  int pad_w = -1;        // width padding when it differs from `pad` (row-expanded stem input)
  int row_expand = 0;    // k > 0: `src` holds the k horizontal taps of a k x k conv per pixel
                         // (DCN columns: k = 9 taps of a 3x3 weight per pixel, kh = kw = 1)
  bool identity = false; // residual added as-is (BasicBlock residual = x): an identity 1x1 weight
  // >= 0: one output phase (pi * 2 + pj) of a ConvTranspose2d(3, stride 2, padding 1) weight
  // [cin][cout][3][3] (masknet.py:21,33): the phase's taps as a kh x kw (= 1 + pi, 1 + pj) conv
  // with no padding over the low-resolution input (tap dy reads row oy + dy: ky = 1 for pi = 0,
  // ky = 2 - 2 dy for pi = 1; the same along x)
  int convt_phase = -1;
};

enum OpKind {
  OP_PREP = 0,
  OP_CONV = 1,
  OP_CONVT_ADD = 2,
  // CenterpointDLA34 (centerpoint_dla.py): elementwise / gather ops on HBM bandwidth
  OP_MAXPOOL = 3,    // MaxPool2d(2, 2, ceil_mode=True) of `src` (Tree.downsample, :199-200)
  OP_DCN = 4,        // DCNv2 sampling: columns [9 taps][C] per pixel of `src` at the offsets /
                     // sigmoid(mask logits) in tensor `add` (18 offsets, 9 logits; :386-392)
  OP_DWCONVT_ADD = 5, // depthwise ConvTranspose2d(2f, f, f//2) of `src` + pad_to_match + `add`
                      // (IDAUp, :446-451); up_s = f, (sy, sx) = (pad_above, pad_left)
  OP_LAYOUT_IN = 6,   // fp32 NCHW input `io` with N channels -> NHWC compute dtype (protonet fpn[0] input,
                      // the YOLACT neck's backbone maps)
  // YOLACT neck and head (planner_yolact_head.cpp)
  OP_BILINEAR_ADD = 7, // out += F.interpolate(src, size of out, "bilinear") in place (feature_pyramid.py:49-50)
  OP_HEAD_SCATTER = 8, // one level's fp32 raw head tensors -> the caller's [A_total, width] outputs (`parts`)
  // ResNet-18 backbone (planner_resnet.cpp): elementwise / window ops on HBM bandwidth (resnet.hip)
  OP_MAXPOOL3S2 = 9,   // MaxPool2d(3, 2, 1) of `src` (floor mode, taps outside the image ignored)
  OP_ADD_RELU = 10,    // out = relu(src + add): the residual add after a tapped bn2 (backbone.py:21-23)
  OP_STORE_F32 = 11    // `src` -> the caller's fp32 NHWC output -1 - out, exactly (a tap that also stays in the arena)
};

// One part of an OP_HEAD_SCATTER: columns [c0, c0 + n) of the fp32 NHWC tensor `src` ([H, W, ldc],
// n = n_ar * width) are, per frame, rows [row0, row0 + H W n_ar) of output `slot` ([A_total, width]
// contiguous): pixel p's n values land at (row0 * width + p * n), which is the reference's
// permute(0, 2, 3, 1).reshape order (prediction_head.py:112-113), aspect ratio innermost.
struct ScatterPart {
  int src, c0, n, slot, row0, width;
  bool tanh;  // mask coefficients (prediction_head.py:141)
};

struct OpSpec {
  int kind = OP_CONV;
  std::string label;          // human-readable (reference module path)
  std::vector<SegSpec> segs;  // OP_CONV
  int out = -1;               // tensor id (-1 - i = the caller's fp32 output buffer i)
  int N = 0;                  // output channels (GEMM columns before phase expansion)
  int act = 0;                // 0 none, 1 relu, 2 leaky
  // head fusion: weights of several convs stacked along N (names in order, N each)
  std::vector<std::string> stack_w;
  std::vector<int> stack_n;
  // final block-diagonal 1x1 heads: weight j feeds output channels [out_off[j], +n) from
  // input channels [in_off[j], +cin)
  std::vector<int> diag_in_off, diag_out_off;
  // OP_CONVT_ADD (and OP_CONV: `add` >= 0 = tensor added before the activation)
  int src = -1, add = -1, up_s = 0, sy = 0, sx = 0;
  std::string up_w;           // ConvTranspose2d prefix
  int cov_y0 = 0, cov_y1 = 0, cov_x0 = 0, cov_x1 = 0;  // covered target rectangle
  double flops = 0;           // algorithmic FLOPs per frame (2*MAC)
  // OP_CONV with up_s > 0: a phase-scatter GEMM over the (gh, gw) grid of its input whose output
  // pixel (oy, ox) lands at (oy * up_s + sy, ox * up_s + sx) of `out` (no skip tensor when add < 0)
  int gh = 0, gw = 0;
  // a second output tensor (the fused stem + block0.conv1 launch also writes the stem at the even
  // pixels, the block's residual input): placed and kept live like `out`
  int out2 = -1;
  int io = 0;            // OP_LAYOUT_IN: which of the caller's inputs
  bool out_f32 = false;  // OP_CONV into an fp32 arena tensor (TensorSpec::f32): the generic GEMMs' fp32 store
  std::vector<ScatterPart> parts;  // OP_HEAD_SCATTER
};

struct TensorSpec {
  int H, W, C;  // per frame, stored channels (ldc == C)
  bool f32 = false;  // fp32 elements in every compute dtype (the raw head logits)
};

// One of the caller's buffers, per frame: an input is fp32 NCHW [C, H, W]; an output fp32 NHWC
// [H, W, cpad] of which C channels are meaningful.
struct IoSpec {
  int H, W, C, cpad;
};
constexpr int kMaxIO = 8;  // == TV_MAX_IO

struct Plan {
  std::vector<ParamInfo> params;     // reference state_dict order
  std::vector<TensorSpec> tensors;
  std::vector<OpSpec> ops;
  int out_h = 0, out_w = 0, out_c = 0, out_cpad = 0;
  int in_cpad = 0;
  int in_channels = 3;               // channels of one input frame (fp32 NCHW path)
  double flops_per_frame = 0;
  std::set<std::string> names;       // every key of `params`
  // the caller's buffers (build_plan fills one of each from in_channels / desc.in_h, in_w and
  // out_* for the single-input single-output archs); an op's out < 0 is output -1 - out
  std::vector<IoSpec> ins, outs;
  const IoSpec& outspec(int out) const { return outs[-1 - out]; }
};

// Returns 0 or a TV_E* code (with tv_last_error set).
int build_plan(const tv_model_desc& d, Plan* plan);
int build_plan_dla34(const tv_model_desc& d, Plan* plan);  // planner_dla34.cpp
int build_plan_protonet(const tv_model_desc& d, Plan* plan);  // planner_protonet.cpp
// Masknet's parameters (keys prefixed) and its forward over the NHWC tensor `x` ([H, W, F]) appended
// to a plan, the prototypes going to the caller's output `out_slot`; returns their IoSpec
IoSpec append_protonet(Plan& P, const std::string& prefix, int x, int F, int k, int out_slot);
int build_plan_yolact_head(const tv_model_desc& d, Plan* plan);  // planner_yolact_head.cpp
// The neck and head (TV_ARCH_YOLACT_HEAD; the FeaturePyramid alone for TV_ARCH_YOLACT_FPN) of a
// checked desc appended to a plan: parameters, ops and the caller's outputs. `maps` empty: the
// backbone maps are the caller's inputs (one OP_LAYOUT_IN each, sizes from d.map_h / map_w); else
// the plan's NHWC tensors `maps` (d.n_levels of them, d.channels[1 + i] channels) feed the lateral
// convs as they are.
int check_yolact_head_desc(const tv_model_desc& d);
void append_yolact_head(Plan& P, const tv_model_desc& d, const std::vector<int>& maps);
// planner_resnet.cpp: torchvision resnet18's parameters (keys prefixed, no fc) and its forward over
// the staged image tensor `img` (row-expanded for the 7x7 stem, as build_plan's) appended to a
// plan; returns the three tap tensors (layer2.1.bn2, layer3.1.bn2, layer4.1.bn2)
std::vector<int> append_resnet18(Plan& P, const std::string& prefix, int img);
int build_plan_resnet(const tv_model_desc& d, Plan* plan);  // TV_ARCH_RESNET18, TV_ARCH_YOLACT

}  // namespace tv
