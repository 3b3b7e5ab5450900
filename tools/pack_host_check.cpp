// Stand-alone host check of the weight packer (csrc/pack.cpp): packs every op of the largest R18
// case and of the whole-YOLACT case in fp32 / fp16 / bf16 with synthetic weights, no GPU and no
// Python. Meant for a sanitizer build of the host code, from tauv-vision_amd/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//     ../tools/pack_host_check.cpp csrc/pack.cpp csrc/planner.cpp csrc/planner_dla34.cpp \
//     csrc/planner_protonet.cpp csrc/planner_yolact_head.cpp csrc/planner_resnet.cpp csrc/stem.hip \
//     csrc/convt3.hip -o /tmp/pack_host_check && /tmp/pack_host_check
// (stem.hip and convt3.hip hold the host packers stem_fragment_order and convt3_pack). Prints the
// packed bytes and the wall time per (case, precision); exit status 0 when every op packed.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../tauv-vision_amd/csrc/pack.h"

namespace tv {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tv

using namespace tv;

static int pack_all(const char* what, tv_model_desc d, int dtype) {
  d.compute_dtype = dtype;
  Plan plan;
  if (build_plan(d, &plan)) return std::printf("%s: build_plan: %s\n", what, g_err.c_str()), 1;
  // synthetic weights in the plan's own layout (running_var must be positive)
  std::vector<std::vector<float>> store;
  HostWeights host_w;
  uint32_t lcg = 12345;
  for (const ParamInfo& p : plan.params) {
    int64_t n = 1;
    for (int64_t s : p.shape) n *= s;
    if (p.name.size() > 19 && p.name.compare(p.name.size() - 19, 19, "num_batches_tracked") == 0) continue;
    store.emplace_back((size_t)n);
    const bool var = p.name.size() > 11 && p.name.compare(p.name.size() - 11, 11, "running_var") == 0;
    for (float& v : store.back()) {
      lcg = lcg * 1664525u + 1013904223u;
      v = (float)(lcg >> 8) / (float)(1 << 24) - (var ? -0.5f : 0.5f);
    }
    host_w[p.name] = {store.back().data(), n};
  }
  // the stem op as Engine::configure finds it: the stride-1 row-expanded 7x7 conv after the staging op
  int stem_op = -1;
  if (dtype != F32 && plan.ops.size() > 1 && plan.ops[0].kind == OP_PREP && plan.ops[1].kind == OP_CONV &&
      plan.ops[1].segs.size() == 1 && plan.ops[1].segs[0].row_expand == 7 && plan.ops[1].segs[0].stride == 1 &&
      plan.ops[1].N <= 128)
    stem_op = 1;
  const auto t0 = std::chrono::steady_clock::now();
  size_t bytes = 0, extra = 0;
  for (size_t i = 0; i < plan.ops.size(); ++i) {
    HostPacked hp;
    if (pack_op_host(plan, i, dtype, host_w, stem_op, 1, &hp))
      return std::printf("%s: op %zu: %s\n", what, i, g_err.c_str()), 1;
    bytes += hp.w.size() + hp.bias.size() * sizeof(float);
    extra += hp.w_ct3.size() + hp.head_w.size() + hp.head_b.size() * sizeof(float);
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("%s dtype %d: %zu ops, %zu weight + bias bytes, %zu fragment bytes, %.1f ms\n", what, dtype,
              plan.ops.size(), bytes, extra, ms);
  return 0;
}

int main(int argc, char** argv) {  // an argument: that dtype only (0 fp32, 1 fp16, 2 bf16)
  tv_model_desc r18{};  // Centernet(DLABackbone([2] * 5, [128] * 6, 2)), heads [4, 2, 2], 480 x 640
  r18.n_levels = 5;
  for (int i = 0; i < 5; ++i) r18.heights[i] = 2;
  for (int i = 0; i < 6; ++i) r18.channels[i] = 128;
  r18.downsamples = 2;
  r18.n_heads = 3;
  r18.head_channels[0] = 4, r18.head_channels[1] = 2, r18.head_channels[2] = 2;
  r18.in_h = 480, r18.in_w = 640;
  r18.arch = TV_ARCH_CENTERNET;
  tv_model_desc yo{};  // whole YOLACT: ResNet-18, F = 256, 2 extra levels, 7 classes, 8 prototypes, 2 aspect ratios
  yo.arch = TV_ARCH_YOLACT;
  yo.in_h = 149, yo.in_w = 77;
  yo.n_levels = 3;
  yo.channels[0] = 256, yo.channels[1] = 128, yo.channels[2] = 256, yo.channels[3] = 512;
  yo.heights[0] = 1;  // one shared prediction-head layer, no extra classification / box / mask layers
  yo.downsamples = 2;
  yo.n_heads = 2;
  yo.head_channels[0] = 8, yo.head_channels[1] = 7;
  yo.n_aspect_ratios = 2;
  int rc = 0;
  for (int dtype : {F32, F16, BF16})
    if (argc < 2 || std::atoi(argv[1]) == dtype)
      rc |= pack_all("r18_c128_480x640", r18, dtype) | pack_all("yolact_149x77", yo, dtype);
  return rc;
}
