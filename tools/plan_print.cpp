// Stand-alone dump of the planners' output (csrc/planner*.cpp): every field of the Plan of a fixed
// list of model descs, odd-sized on purpose, in fp32 / fp16 / bf16, and the return code and error
// text of a list of refused descs. No GPU and no Python. Two builds of the planners lower alike
// exactly when their dumps are byte-identical, so build it before and after a planner change and
// diff; it is also the planners' entry for a sanitizer build of the host code, from tauv-vision_amd/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//     ../tools/plan_print.cpp csrc/planner.cpp csrc/planner_dla34.cpp csrc/planner_protonet.cpp \
//     csrc/planner_yolact_head.cpp csrc/planner_resnet.cpp -o /tmp/plan_print && /tmp/plan_print
// Exit status 0 when every listed desc planned and every refusal was refused. No CenterNet desc
// reaches "pad_to_match would yield a smaller tensor": every level is ceil(H / 2) of the one above,
// so an upsampled map is never smaller than its target; that refusal is not in the list.
#include <cstdio>

#include "../tauv-vision_amd/csrc/planner.h"

namespace tv {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tv

using namespace tv;

static const char* s(const std::string& v) { return v.c_str(); }

static void print_plan(const Plan& P) {
  std::printf("in_cpad %d in_channels %d out %d %d %d %d flops_per_frame %a\n", P.in_cpad, P.in_channels, P.out_h,
              P.out_w, P.out_c, P.out_cpad, P.flops_per_frame);
  for (const IoSpec& io : P.ins) std::printf("in %d %d %d %d\n", io.H, io.W, io.C, io.cpad);
  for (const IoSpec& io : P.outs) std::printf("out %d %d %d %d\n", io.H, io.W, io.C, io.cpad);
  for (const ParamInfo& p : P.params) {
    std::printf("param %s%s [", s(p.name), P.names.count(p.name) ? "" : " (not in names)");
    for (int64_t v : p.shape) std::printf(" %lld", (long long)v);
    std::printf(" ]\n");
  }
  std::printf("names %zu\n", P.names.size());
  for (size_t i = 0; i < P.tensors.size(); ++i)
    std::printf("tensor %zu: %d %d %d f32 %d\n", i, P.tensors[i].H, P.tensors[i].W, P.tensors[i].C, (int)P.tensors[i].f32);
  for (size_t i = 0; i < P.ops.size(); ++i) {
    const OpSpec& o = P.ops[i];
    // `act` is read for OP_CONV alone, and the ops that move or pool data may leave it unset
    const bool has_act = o.kind != OP_PREP && o.kind != OP_CONVT_ADD && o.kind != OP_MAXPOOL && o.kind != OP_DCN &&
                         o.kind != OP_DWCONVT_ADD && o.kind != OP_LAYOUT_IN;
    std::printf("op %zu: kind %d '%s' out %d out2 %d N %d act %d src %d add %d up_s %d sy %d sx %d up_w '%s' cov %d %d %d %d "
                "g %d %d io %d out_f32 %d flops %a\n",
                i, o.kind, s(o.label), o.out, o.out2, o.N, has_act ? o.act : 0, o.src, o.add, o.up_s, o.sy, o.sx, s(o.up_w),
                o.cov_y0, o.cov_y1, o.cov_x0, o.cov_x1, o.gh, o.gw, o.io, (int)o.out_f32, o.flops);
    for (const SegSpec& g : o.segs)
      std::printf("  seg src %d w '%s' bn '%s' ci0 %d cin %d k %d %d stride %d pad %d pad_w %d row_expand %d identity %d "
                  "convt_phase %d\n",
                  g.src, s(g.wname), s(g.bn), g.ci0, g.cin, g.kh, g.kw, g.stride, g.pad, g.pad_w, g.row_expand,
                  (int)g.identity, g.convt_phase);
    for (size_t j = 0; j < o.stack_w.size(); ++j) std::printf("  stack '%s' %d\n", s(o.stack_w[j]), o.stack_n[j]);
    for (size_t j = 0; j < o.diag_in_off.size(); ++j) std::printf("  diag %d %d\n", o.diag_in_off[j], o.diag_out_off[j]);
    for (const ScatterPart& p : o.parts)
      std::printf("  part src %d c0 %d n %d slot %d row0 %d width %d tanh %d\n", p.src, p.c0, p.n, p.slot, p.row0, p.width,
                  (int)p.tanh);
  }
}

static int n_bad = 0;

// plans `d` in one dtype (`refused`: must be turned down) and prints the plan or the refusal
static void run(const char* what, tv_model_desc d, int dtype, bool refused = false) {
  d.compute_dtype = dtype;
  Plan plan;
  g_err.clear();
  const int rc = build_plan(d, &plan);
  std::printf("== %s dtype %d: rc %d%s%s\n", what, dtype, rc, rc ? " error: " : "", rc ? g_err.c_str() : "");
  if (!rc) print_plan(plan);
  n_bad += (rc != 0) != refused;
}

static tv_model_desc centernet(int arch, int L, const int* heights, const int* ch, int downsamples, int h, int w) {
  tv_model_desc d{};
  d.arch = arch;
  d.n_levels = L;
  for (int i = 0; i < L; ++i) d.heights[i] = heights[i];
  for (int i = 0; i <= L; ++i) d.channels[i] = ch[i];
  d.downsamples = downsamples;
  d.in_h = h, d.in_w = w;
  return d;
}

static tv_model_desc with_heads(tv_model_desc d, int n, int a, int b = 0, int c = 0) {
  d.n_heads = n;
  d.head_channels[0] = a, d.head_channels[1] = b, d.head_channels[2] = c;
  return d;
}

int main() {
  const int h5[5] = {2, 2, 2, 2, 2}, c5[6] = {128, 128, 128, 128, 128, 128};
  const int h3[3] = {1, 2, 3}, c3[4] = {16, 32, 64, 128};
  const int h8[1] = {8}, c8[2] = {16, 16}, c18[4] = {16, 18, 64, 128};
  tv_model_desc dla = with_heads(tv_model_desc{}, 3, 4, 2, 2);
  dla.arch = TV_ARCH_DLA34;
  tv_model_desc proto = with_heads(tv_model_desc{}, 1, 16);
  proto.arch = TV_ARCH_PROTONET;
  proto.channels[0] = 64;
  proto.in_h = 9, proto.in_w = 17;
  // neck + head: F = 256 over backbone maps of 128 / 256 / 512 channels, 2 extra levels, 2 aspect ratios
  tv_model_desc head = with_heads(tv_model_desc{}, 2, 8, 7);
  head.n_levels = head.n_maps = 3;
  const int hc[4] = {256, 128, 256, 512}, mh[3] = {19, 10, 5}, mw[3] = {10, 5, 3}, sep[4] = {1, 1, 2, 1};
  for (int i = 0; i < 4; ++i) head.channels[i] = hc[i];
  for (int i = 0; i < 3; ++i) head.map_h[i] = mh[i], head.map_w[i] = mw[i];
  head.downsamples = 2;
  head.n_aspect_ratios = 2;
  head.heights[0] = 1;  // the three final convs stacked; `sep`: a branch of its own each
  for (int dtype = 0; dtype < 3; ++dtype) {
    for (int arch : {TV_ARCH_CENTERNET, TV_ARCH_CENTERNET_BACKBONE}) {
      run("centernet 5x2 c128 ds2 480x640", with_heads(centernet(arch, 5, h5, c5, 2, 480, 640), 3, 4, 2, 2), dtype);
      run("centernet {1,2,3} ds1 97x131", with_heads(centernet(arch, 3, h3, c3, 1, 97, 131), 1, 3), dtype);
      run("centernet {1,2,3} ds0 97x131", with_heads(centernet(arch, 3, h3, c3, 0, 97, 131), 1, 3), dtype);
    }
    for (int hw : {100 * 1000 + 104, 33 * 1000 + 47, 32 * 1000 + 32, 31 * 1000 + 31}) {
      dla.in_h = hw / 1000, dla.in_w = hw % 1000;
      run("dla34", dla, dtype, dla.in_h < 32);
    }
    run("protonet F64 k16 9x17", proto, dtype);
    run("protonet with two heads", with_heads(proto, 2, 16, 4), dtype, true);
    for (int arch : {TV_ARCH_YOLACT_HEAD, TV_ARCH_YOLACT_FPN, TV_ARCH_RESNET18, TV_ARCH_YOLACT}) {
      tv_model_desc d = head;
      d.arch = arch;
      if (arch == TV_ARCH_RESNET18 || arch == TV_ARCH_YOLACT) d.in_h = 149, d.in_w = 77;
      run("yolact stacked finals", d, dtype);
      for (int i = 0; i < 4; ++i) d.heights[i] = sep[i];
      if (arch != TV_ARCH_RESNET18) run("yolact separate branches", d, dtype);
      d.n_maps = 2;  // read by the neck + head archs alone
      if (arch == TV_ARCH_YOLACT_HEAD || arch == TV_ARCH_YOLACT_FPN) run("yolact n_maps 2", d, dtype, true);
      d.n_levels = 0;
      if (arch == TV_ARCH_YOLACT_HEAD) run("yolact n_levels 0", d, dtype, true);
    }
    run("centernet n_levels 0", with_heads(centernet(TV_ARCH_CENTERNET, 0, h3, c3, 1, 97, 131), 1, 3), dtype, true);
    run("centernet channels 18", with_heads(centernet(TV_ARCH_CENTERNET, 3, h3, c18, 1, 97, 131), 1, 3), dtype, true);
    run("centernet height 8", with_heads(centernet(TV_ARCH_CENTERNET, 1, h8, c8, 0, 64, 64), 1, 3), dtype, true);
  }
  for (int arch = 0; arch < 8; ++arch) {  // every planner turns an unknown compute dtype down
    tv_model_desc d = arch == TV_ARCH_DLA34 ? dla : arch == TV_ARCH_PROTONET ? proto : head;
    if (arch == TV_ARCH_CENTERNET || arch == TV_ARCH_CENTERNET_BACKBONE)
      d = with_heads(centernet(arch, 3, h3, c3, 1, 97, 131), 1, 3);
    d.arch = arch;
    if (!d.in_h) d.in_h = 149, d.in_w = 77;
    run("compute_dtype 7", d, 7, true);
  }
  return n_bad != 0;
}
