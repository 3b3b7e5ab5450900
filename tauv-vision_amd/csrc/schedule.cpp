// Engine::plan_schedule: every decision about one (batch) workspace, with no HIP call: execution
// order, arena layout, launch geometry, the kernel each op runs (its Route), split-K, launch groups.
// The kernel choice is a fixed sequence of passes; each names the routes it may take an op from.
#include "engine.h"

#include <algorithm>
#include <cassert>

namespace tv {

namespace {

struct Planner {
  const Engine& e;
  const int B;  // frames of this workspace
  Workspace& ws;
  const Plan& plan = e.plan;
  const int dtype = e.dtype, esz = dtype_size(e.dtype);
  const size_t nops = e.plan.ops.size();
  // Launch grouping only on the latency path (B <= lat_group_max_b frames per launch): at B = 32
  // per slice the other slice fills the CUs these small layers leave idle, and the reordering
  // measured 0.5% slower there (profiles/r4y); at B = 1 it took 1.43 -> 1.35 ms.
  const bool grouping = e.lat_group && B <= e.lat_group_max_b;
  std::vector<std::vector<KStep>> op_ks{nops};  // per op: its k-step descriptors when each has one
  std::vector<char> lat_ok = std::vector<char>(nops, 0);  // ... and every k-step lies in one tap (mode 0)

  Route& kind(size_t i) { return ws.route[i].kind; }
  bool generic(size_t i) { return kind(i) == Route::ConvPipe || kind(i) == Route::ConvIgemm; }
  char* at(int tensor) const { return reinterpret_cast<char*>(kArenaTag + ws.off[tensor]); }

  // Dependency levels: a conv / ConvT + add op runs one level after the last producer of a tensor
  // it reads (the MultiIDAUp wavefront: IDAUp i+1's step at a level needs only IDAUp i's output
  // there and its own previous step, dla.py:265-284, 377-390; the IDAUpReverse projections need
  // only MultiIDAUp's outputs); every other op (staging, the fp32-output heads, DCN sampling,
  // pooling, depthwise up-sampling) is a barrier after everything before it. Ops then run by
  // level (plan order within one), and the arena's lifetimes are counted in levels, so that ops
  // of one level may run in one launch.
  void plan_levels() {
    ws.level.assign(nops, 0);
    std::vector<int> prod(plan.tensors.size(), -1);
    int barrier = -1, maxlev = -1;
    for (size_t i = 0; i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      int lv;
      if (!grouping) {
        lv = (int)i;
      } else if ((op.kind == OP_CONV || op.kind == OP_CONVT_ADD) && op.out >= 0) {
        lv = barrier + 1;
        auto after = [&](int t) { if (t >= 0 && prod[t] >= 0) lv = std::max(lv, prod[t] + 1); };
        for (const SegSpec& sg : op.segs) after(sg.src);
        after(op.src);
        after(op.add);
      } else {
        lv = maxlev + 1;
        barrier = lv;
      }
      ws.level[i] = lv;
      maxlev = std::max(maxlev, lv);
      if (op.out >= 0) prod[op.out] = std::max(prod[op.out], lv);
      if (op.out2 >= 0) prod[op.out2] = std::max(prod[op.out2], lv);
    }
    ws.order.resize(nops);
    for (size_t i = 0; i < nops; ++i) ws.order[i] = (int)i;
    std::stable_sort(ws.order.begin(), ws.order.end(), [&](int a, int b) { return ws.level[a] < ws.level[b]; });
  }

  // DCNv2 sampling (op i) + its column GEMM (op i + 1) that run as one fused kernel (dcn.hip)
  bool dcn_fusable(size_t i) const {
    if (dtype == F32 || i + 1 >= nops) return false;
    const OpSpec& d = plan.ops[i];
    const OpSpec& g = plan.ops[i + 1];
    if (d.kind != OP_DCN || g.kind != OP_CONV || g.segs.size() != 1 || g.segs[0].src != d.out ||
        g.segs[0].row_expand != 9 || g.out < 0 || g.add >= 0)
      return false;
    const TensorSpec& xt = plan.tensors[d.src];
    return dcn_gemm_supported((long)B * xt.H * xt.W, xt.C, g.N, xt.C, plan.tensors[d.add].C, plan.tensors[g.out].C,
                              e.packed[i + 1].Kpad) &&
           g.segs[0].cin == xt.C;
  }

  // The routes the op kind alone decides, the stem pair Engine::create found, and the DCN sampling ops
  // a fused kernel absorbs (here, because their column tensor then needs no arena space; pass_dcn
  // builds the launch). Convs start as ConvIgemm: pass_generic looks at them first.
  void fixed_routes() {
    ws.route.assign(nops, OpRoute{});
    for (size_t i = 0; i < nops; ++i) {
      switch (plan.ops[i].kind) {
        case OP_PREP: kind(i) = e.stem_op >= 0 ? Route::StagingInStem : Route::Staging; break;
        case OP_LAYOUT_IN: kind(i) = Route::LayoutIn; break;
        case OP_MAXPOOL: kind(i) = Route::MaxPool; break;
        case OP_DCN: kind(i) = dcn_fusable(i) ? Route::DcnInFused : Route::DcnSample; break;
        case OP_DWCONVT_ADD: kind(i) = Route::DwConvTAdd; break;
        case OP_BILINEAR_ADD: kind(i) = Route::BilinearAdd; break;
        case OP_HEAD_SCATTER: kind(i) = Route::HeadScatter; break;
        case OP_MAXPOOL3S2: kind(i) = Route::MaxPool3S2; break;
        case OP_ADD_RELU: kind(i) = Route::AddRelu; break;
        case OP_STORE_F32: kind(i) = Route::StoreF32; break;
      }
    }
    if (e.stem_op >= 0) kind(e.stem_op) = e.ss2_op >= 0 ? Route::StemInS2 : Route::Stem;
    if (e.ss2_op >= 0) kind(e.ss2_op) = Route::StemS2;
  }

  // 0. stem7s2_pool (the max-pool op from MaxPool3S2, its stem conv from the initial ConvIgemm, their
  // staging op from Staging): the ResNet stem pair Engine::create found runs staging, conv, ReLU and
  // pooling as one launch on the pool's op (resnet.hip). Before plan_arena: neither the staged image
  // nor the conv output then needs arena space.
  void pass_stem_pool() {
    if (e.rstem_op < 0) return;
    const size_t i = (size_t)e.rstem_op;
    if (kind(i - 1) != Route::Staging || kind(i) != Route::ConvIgemm || kind(i + 1) != Route::MaxPool3S2) return;
    kind(i - 1) = Route::StagingInStem;
    kind(i) = Route::StemInPool;
    kind(i + 1) = Route::StemPool;
  }

  // Liveness-planned arena: a tensor lives from its producing op's level to its last reader's;
  // first-fit placement of each new tensor into the gaps left by dead ones. The outputs of
  // StagingInStem, StemInS2, StemInPool and DcnInFused ops are never stored and get no space.
  void plan_arena() {
    const size_t nt = plan.tensors.size();
    std::vector<int> last(nt, -1);
    for (size_t i = 0; i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      auto used = [&](int t) { if (t >= 0) last[t] = std::max(last[t], ws.level[i]); };
      for (int t : {op.out, op.out2, op.src, op.add}) used(t);
      for (const SegSpec& s : op.segs) used(s.src);
      for (const ScatterPart& q : op.parts) used(q.src);
      // the fused DCNv2 kernel (dcn.hip) samples x and reads the offset / mask tensor while it runs
      // the column GEMM (op i): both stay live through it
      if (op.kind == OP_CONV && i > 0 && plan.ops[i - 1].kind == OP_DCN && op.segs.size() == 1 &&
          op.segs[0].src == plan.ops[i - 1].out)
        for (int t : {plan.ops[i - 1].src, plan.ops[i - 1].add}) used(t);
    }
    ws.off.assign(nt, 0);
    struct Live { size_t off, size; int last; };
    std::vector<Live> live;
    std::vector<char> placed(nt, 0);  // a tensor written by several ops (ConvT phases) is placed once
    size_t peak = 0;
    auto place = [&](int tid) {
      if (placed[tid]) return;
      placed[tid] = 1;
      const TensorSpec& t = plan.tensors[tid];
      size_t sz = align_up((size_t)B * t.H * t.W * t.C * (t.f32 ? 4 : esz), 256);
      std::sort(live.begin(), live.end(), [](const Live& a, const Live& b) { return a.off < b.off; });
      size_t pos = 0;
      for (const Live& l : live) {
        if (pos + sz <= l.off) break;
        pos = std::max(pos, l.off + l.size);
      }
      ws.off[tid] = pos;
      live.push_back({pos, sz, last[tid]});
      peak = std::max(peak, pos + sz);
    };
    for (const int i : ws.order) {
      const OpSpec& op = plan.ops[i];
      live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return l.last < ws.level[i]; }), live.end());
      if (op.out < 0 || kind(i) == Route::StagingInStem || kind(i) == Route::StemInS2 || kind(i) == Route::StemInPool ||
          kind(i) == Route::DcnInFused)
        continue;
      place(op.out);
      if (op.out2 >= 0) place(op.out2);
    }
    ws.bytes = peak;
  }

  // The GEMM view of every conv / ConvT + add op (DLA34's bandwidth ops have none)
  void conv_geometry() {
    ws.params.assign(nops, ConvParams{});
    for (size_t i = 0; i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if (op.kind != OP_CONV && op.kind != OP_CONVT_ADD) continue;
      ConvParams& p = ws.params[i];
      const Packed& pk = e.packed[i];
      p.Kpad = pk.Kpad;
      if (op.kind == OP_CONV) {
        int kbase = 0;
        p.act = op.act;  // (a ConvT + add has no activation: the planner leaves its `act` unset)
        p.nseg = (int)op.segs.size();
        for (size_t s = 0; s < op.segs.size(); ++s) {
          const SegSpec& sg = op.segs[s];
          const TensorSpec& t = plan.tensors[sg.src];
          p.seg[s] = ConvSegment{at(sg.src), t.H, t.W, t.C, t.C, sg.kh, sg.kw, sg.stride, sg.pad,
                                 sg.pad_w >= 0 ? sg.pad_w : sg.pad, pk.seg_ksteps[s], kbase};
          kbase += pk.seg_ksteps[s];
        }
        p.Ho = op.up_s ? op.gh : op.out >= 0 ? plan.tensors[op.out].H : plan.outspec(op.out).H;
        p.Wo = op.up_s ? op.gw : op.out >= 0 ? plan.tensors[op.out].W : plan.outspec(op.out).W;
        p.N = op.N;
        p.out = op.out >= 0 ? at(op.out) : nullptr;  // the caller's fp32 output: patched per call
        p.out_ldc = op.out >= 0 ? plan.tensors[op.out].C : plan.outspec(op.out).cpad;
        p.ntiles = pk.Npad / kTile;
      } else {
        const TensorSpec& src = plan.tensors[op.src];
        p.nseg = 1;
        p.seg[0] = ConvSegment{at(op.src), src.H, src.W, src.C, src.C, 1, 1, 1, 0, 0, pk.seg_ksteps[0], 0};
        p.Ho = src.H; p.Wo = src.W;
        p.N = op.up_s * op.up_s * op.N;
        p.out = at(op.out); p.out_ldc = plan.tensors[op.out].C;
        p.ntiles = (p.N + kTile - 1) / kTile;
      }
      p.M = B * p.Ho * p.Wo;
      p.mtiles = (p.M + kTile - 1) / kTile;
      if (op.up_s) {  // phase scatter into the high-resolution output (ConvT + add, protonet ConvT phases)
        p.up_s = op.up_s; p.up_cout = op.N; p.sy = op.sy; p.sx = op.sx;
        p.tH = plan.tensors[op.out].H; p.tW = plan.tensors[op.out].W;
        p.add = op.add >= 0 ? at(op.add) : nullptr;
        p.add_ldc = op.add >= 0 ? plan.tensors[op.add].C : 0;
      }
    }
  }

  // 1. generic (from the initial ConvIgemm): the pipelined implicit GEMM (conv_pipe.hip, 256-pixel
  // tiles) when every k-step of the layer has a descriptor and pipe_mode allows, else conv_igemm
  void pass_generic() {
    const int BK = 128 / esz;
    for (size_t i = 0; i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if ((op.kind != OP_CONV && op.kind != OP_CONVT_ADD) || kind(i) != Route::ConvIgemm) continue;
      ConvParams& p = ws.params[i];
      std::vector<KStep> ks;
      bool ok = true;
      for (int s = 0; s < p.nseg && ok; ++s) {
        const ConvSegment& sg = p.seg[s];
        for (int kk = 0; kk < sg.ksteps; ++kk) {
          KStep d{};
          d.src = sg.src;
          d.seg = s;
          d.H = sg.H; d.W = sg.W; d.ldc = sg.ldc; d.stride = sg.stride;
          d.pad_h = sg.pad; d.pad_w = sg.pad_w; d.kh = sg.kh; d.kw = sg.kw;
          d.kw_inv = 1.0f / (float)sg.kw;
          const int kel = kk * BK;
          const int vec = 16 / esz;
          if (sg.C % BK == 0 && sg.kh * sg.kw <= 32) {
            const int tap = kel / sg.C;
            d.mode = 0; d.tap = tap;
            d.off = ((long long)(tap / sg.kw) * sg.W + tap % sg.kw) * sg.ldc + kel % sg.C;
          } else if (sg.C < BK && sg.C % vec == 0 && (sg.kh * sg.kw + 8) * (sg.C / vec) < (1 << 16)) {
            d.mode = 1; d.q0 = kel / vec; d.cpt = sg.C / vec;
            d.cpt_inv = 1.0f / (float)d.cpt;
          } else {
            ok = false;
            break;
          }
          ks.push_back(d);
        }
      }
      if (!ok) continue;
      lat_ok[i] = !ks.empty() && std::all_of(ks.begin(), ks.end(), [](const KStep& d) { return d.mode == 0; });
      const int mt = (p.M + kPipeTileM - 1) / kPipeTileM;
      const bool big = (long)mt * p.ntiles >= 256;
      if (e.pipe_mode == 1 || (e.pipe_mode < 0 && big)) {
        kind(i) = Route::ConvPipe;
        p.nks = (int)ks.size();
        p.mtiles = mt;
      }
      op_ks[i] = std::move(ks);
    }
  }

  // 2. conv3x3 (from ConvPipe / ConvIgemm): the persistent halo-tile 3x3 kernel (conv3x3.hip):
  // 3x3 / stride 1 / pad 1, one input of 64 / 128 / 256 channels, fp16/bf16, 16-byte aligned
  // channel slices, byte offsets within 2^31.
  // A second segment is accepted when it is ResidualBlock's 1x1 conv_residual (128 channels,
  // stride 1 or 2, ReLU after the sum): one extra k-step per channel block (RES).
  // (or DLA-34 BasicBlock's identity residual: 64 / 128 / 256 channels, an identity 1x1)
  // (a residual narrower than the 3x3 input — DLA-34 Tree's `project` of the pooled bottom, C/2
  // channels — reads zeros with zero weights in its missing channel blocks)
  void pass_conv3x3() {
    for (size_t i = 0; e.conv3_mode && dtype != F32 && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      ConvParams& p = ws.params[i];
      if (!generic(i) || op.kind != OP_CONV || op.out < 0 || op.out_f32 || op.add >= 0) continue;
      const bool res2 = op.segs.size() == 2 && op.segs[1].kh == 1 && op.segs[1].kw == 1 && op.segs[1].pad == 0 &&
                        p.seg[1].C <= p.seg[0].C && p.seg[1].C % 32 == 0 && p.seg[1].ldc % 8 == 0 && op.act == 1 &&
                        (size_t)p.seg[1].H * p.seg[1].W * p.seg[1].ldc * esz < (1ull << 31) &&
                        p.seg[1].H >= (p.Ho - 1) * p.seg[1].stride + 1 && p.seg[1].W >= (p.Wo - 1) * p.seg[1].stride + 1;
      if (op.segs.size() != 1 && !res2) continue;
      const SegSpec& sg = op.segs[0];
      const ConvSegment& cs = p.seg[0];
      const int pw = sg.pad_w >= 0 ? sg.pad_w : sg.pad;
      const size_t src_bytes = (size_t)B * cs.H * cs.W * cs.ldc * esz;
      if (!(sg.kh == 3 && sg.kw == 3 && sg.stride == 1 && sg.pad == 1 && pw == 1 && !sg.row_expand &&
            (cs.C == 128 || cs.C == 256 || cs.C == 64) &&
            cs.ldc % 8 == 0 && p.out_ldc % 8 == 0 && p.out_coff % 8 == 0 && src_bytes < (1ull << 31) &&
            p.ntiles * 128 <= kConv3MaxN && p.act >= 0 && p.act <= 2 && cs.H * cs.W >= e.conv3_min_pix &&
            (size_t)cs.H * cs.W * p.out_ldc * esz < (1ull << 31)))
        continue;
      const int res = res2 ? 1 : 0;
      const bool heads = op.act >= 1 && !res && i + 1 < nops && !plan.ops[i + 1].diag_in_off.empty();
      int nw = 8, tw = 0, mt = 0, ni = 4;
      long t4 = 0;
      auto geometry = [&](int nwv) {  // tile width, tiles and channel-tile choice for a workgroup size
        const int slots = nwv == 4 ? 2 * e.cu_count : e.cu_count;  // resident workgroups
        const int t16 = conv3x3_tiles(B, cs.H, cs.W, 16, nwv), t32 = conv3x3_tiles(B, cs.H, cs.W, 32, nwv);
        tw = e.c3_tw_force ? e.c3_tw_force : t32 <= t16 ? 32 : 16;
        mt = tw == 32 ? t32 : t16;
        // 64-channel half tiles when the last round of 128-channel tiles would leave most CUs
        // idle: a half tile costs ~c3_half_cost of a full one (two work units per tile)
        t4 = (long)mt * p.ntiles;
        const long r4 = (t4 + slots - 1) / slots, r2 = (2 * t4 + slots - 1) / slots;
        ni = e.c3_ni_force ? e.c3_ni_force : (e.c3_half_cost > 0 && e.c3_half_cost * r2 < 100 * r4) ? 2 : 4;
        if (p.N <= 64) ni = 2;  // one 64-channel half tile holds every output channel
        if (heads) ni = 4;      // the stacked heads (fused 1x1 epilogue) keep 128-channel tiles
      };
      geometry(8);
      // two 4-wave workgroups per CU (256-pixel tiles) for the plain 128-channel-input convs that
      // run 64-channel half tiles. Measured (profiles/r3c): the R18 60x80 layers 1.000 -> 0.916 ms
      // per slice; on the dominant 120x160 layer (128-channel tiles) 1.432 -> 1.506 ms, so those
      // keep one 8-wave workgroup per CU
      if (ni == 2 && e.c3_nw_mode != 8 && !res && !heads && cs.C == 128 && p.ntiles <= 2) {
        nw = 4;
        geometry(4);
        ni = 2;
      }
      const int slots = nw == 4 ? 2 * e.cu_count : e.cu_count;
      const long total = (ni == 2 && p.N <= 64) ? t4 : t4 * (4 / ni);
      int grid = (int)std::min<long>(total, slots);
      // XCD-aware contiguous ranges need a multiple of 8 workgroups; rounding down is only
      // worth it when every workgroup still gets several units (measured at B=1: 20 units on
      // 16 workgroups ran two rounds, 29 us instead of 18)
      if (grid >= 8 && total > 2L * slots) grid -= grid % 8;
      ws.route[i].geom = C3Geom{tw, grid, res, ni, nw};
      kind(i) = Route::Conv3x3;
      p.mtiles = mt;
    }
  }

  // 3. conv3x3s2 (from ConvPipe / ConvIgemm): the persistent stride-2 3x3 kernel (conv3x3s2.hip): 128 -> 128
  // channels, fp16/bf16, from s2_min_tiles 512-pixel tiles (measured at B=1: faster on the small levels too)
  void pass_conv3x3s2() {
    for (size_t i = 0; e.s2_mode && dtype != F32 && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      ConvParams& p = ws.params[i];
      if (!generic(i) || op.kind != OP_CONV || op.segs.size() != 1 || op.out < 0 || op.out_f32 || op.add >= 0) continue;
      const SegSpec& sg = op.segs[0];
      const ConvSegment& cs = p.seg[0];
      const int pw = sg.pad_w >= 0 ? sg.pad_w : sg.pad;
      const size_t frame_bytes = (size_t)cs.H * cs.W * cs.ldc * esz;
      const int mt = conv3x3s2_tiles(B, p.Ho, p.Wo);
      if (!(sg.kh == 3 && sg.kw == 3 && sg.stride == 2 && sg.pad == 1 && pw == 1 && !sg.row_expand && cs.C == 128 &&
            p.N == 128 && p.ntiles == 1 && cs.ldc % 8 == 0 && p.out_ldc % 8 == 0 && frame_bytes < (1ull << 31) &&
            mt >= (e.s2_min_tiles >= 0 ? e.s2_min_tiles : e.cu_count)))
        continue;
      int grid = std::min(mt, e.cu_count);
      if (grid >= 8 && mt > 2 * e.cu_count) grid -= grid % 8;
      ws.route[i].geom = S2Geom{grid};
      kind(i) = Route::Conv3x3S2;
      p.mtiles = mt;
    }
  }

  // 4. conv_small (from ConvPipe / ConvIgemm): narrow-channel 3x3 convs (16 / 32 input channels)
  void pass_conv_small() {
    for (size_t i = 0; dtype != F32 && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if (!generic(i) || op.kind != OP_CONV || op.segs.size() != 1 || op.out < 0 || op.out_f32 || op.add >= 0 || op.up_s)
        continue;
      const SegSpec& sg = op.segs[0];
      const ConvParams& p = ws.params[i];
      if (sg.kh == 3 && sg.kw == 3 && sg.pad == 1 && (sg.pad_w < 0 || sg.pad_w == 1) && !sg.row_expand &&
          conv_small_supported(p.seg[0].C, op.N, sg.stride, p.seg[0].ldc, p.out_ldc) && p.N == op.N)
        kind(i) = Route::ConvSmall;
    }
  }

  // 5. fused DCN (from ConvPipe / ConvIgemm): the column GEMM after a DcnInFused op (fixed_routes)
  // launches sampling + GEMM as one kernel (dcn.hip)
  // dcn_gemm64 split-K: a layer whose (pixel, channel) tiles fill at most half the CUs (DLA-34 at
  // B=1: a 30x40 256-channel layer is 38 tiles of 36 k-steps, each k-step a chain of corner gathers)
  // runs ksplit workgroups per tile over tap ranges; their fp32 partials meet in dslab
  void pass_dcn() {
    for (size_t i = 0; i + 1 < nops; ++i) {
      if (kind(i) != Route::DcnInFused) continue;
      assert(generic(i + 1));  // (its column tensor has no arena space: nothing else may have taken the GEMM)
      const OpSpec& d = plan.ops[i];
      const OpSpec& g = plan.ops[i + 1];
      const TensorSpec& xt = plan.tensors[d.src];
      DcnParams q{};
      q.x = at(d.src); q.B = B; q.H = xt.H; q.W = xt.W; q.C = xt.C; q.ldx = xt.C;
      q.om = at(d.add); q.om_ldc = plan.tensors[d.add].C;
      q.Kpad = e.packed[i + 1].Kpad; q.act = g.act; q.N = g.N;
      q.out = at(g.out); q.out_ldc = plan.tensors[g.out].C;
      if (e.dcn_split_max >= 2 && (e.dcn64_mode == 1 || e.dcn64_mode == 2) && q.C % 64 == 0) {
        int bn, px;
        dcn64_tile(q, e.dcn64_mode, &bn, &px);
        const long units = ((long)q.B * q.H * q.W + px - 1) / px * (q.N / bn);
        const int ks = (int)std::min<long>(e.dcn_split_max, e.cu_count / std::max(1L, units));
        if (ks >= 2) {
          q.ksplit = ks;
          ws.dcn_slab_floats = std::max(ws.dcn_slab_floats, (size_t)dcn_split_floats(q, e.dcn64_mode, ks));
          ws.dcn_tickets = std::max(ws.dcn_tickets, (size_t)units);
        }
      }
      ws.route[i + 1].geom = q;
      kind(i + 1) = Route::DcnFused;
    }
  }

  // 6. fused heads (from Conv3x3 on 8-wave 128-channel tiles): the stacked 3x3 heads take the
  // block-diagonal 1x1 heads of the next op (from ConvPipe / ConvIgemm: it writes the caller's
  // fp32 output, which no pass before this one accepts) into their epilogue (conv3x3 EPI 1)
  void pass_heads() {
    for (size_t i = 0; e.headfuse_mode && i + 1 < nops; ++i) {
      const OpSpec& h1 = plan.ops[i];
      const OpSpec& h2 = plan.ops[i + 1];
      const Packed& pk2 = e.packed[i + 1];
      ConvParams& p = ws.params[i];
      if (kind(i) != Route::Conv3x3) continue;
      const C3Geom& g = std::get<C3Geom>(ws.route[i].geom);
      if (g.ni != 4 || g.nw != 8 || g.res || !generic(i + 1) || h2.diag_in_off.empty() || !pk2.head_ok ||
          h2.out >= 0 || h2.segs[0].src != h1.out || p.ntiles != h1.N / 128 ||
          (h1.act != 2 && !(h1.act == 1 && plan.tensors[h1.segs[0].src].C == 64)))
        continue;
      const int out_cpad = plan.outspec(h2.out).cpad;
      p.head_ldc = out_cpad;
      for (int t = 0; t < 16; ++t) p.head_row0[t] = pk2.head_row0[t], p.head_nrows[t] = pk2.head_nrows[t];
      // plain stores when the tiles' head rows tile the output columns exactly once (one 128-channel
      // hidden tile per head: a 64-channel backbone's 2C heads); otherwise (a head's 2C = 256 hidden
      // channels, centernet.py:45-50 on the 128-channel "R18" and DLA-34, span two tiles that meet in
      // the output) atomics onto a zeroed output
      std::vector<int> cover(out_cpad, 0);
      bool ok = true;
      for (int t = 0; t < p.ntiles && t < 16; ++t)
        for (int r = 0; r < p.head_nrows[t]; ++r) {
          const int c = p.head_row0[t] + r;
          if (c < 0 || c >= out_cpad) ok = false;
          else ++cover[c];
        }
      for (int c : cover) ok = ok && c == 1;
      p.head_store = ok ? 1 : 0;
      kind(i) = Route::HeadsFused;
      kind(i + 1) = Route::HeadsDone;
    }
  }

  // 7. convt (from ConvPipe / ConvIgemm, the only routes an OP_CONVT_ADD can have): ConvTranspose +
  // pad_to_match + add on convt.hip (fp16/bf16, 128 -> 128 channels)
  void pass_convt() {
    for (size_t i = 0; e.convt_mode && dtype != F32 && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if (!generic(i) || op.kind != OP_CONVT_ADD) continue;
      const TensorSpec& src = plan.tensors[op.src];
      const TensorSpec& tgt = plan.tensors[op.out];
      const TensorSpec& add = plan.tensors[op.add];
      if (!convt_supported(src.C, op.N, src.C, add.C, tgt.C)) continue;
      ConvTParams t{};
      t.src = at(op.src); t.h = src.H; t.w = src.W; t.src_ldc = src.C;
      t.Kpad = e.packed[i].Kpad;
      t.add = at(op.add); t.add_ldc = add.C;
      t.out = at(op.out); t.out_ldc = tgt.C;
      t.B = B; t.s = op.up_s; t.tH = tgt.H; t.tW = tgt.W; t.sy = op.sy; t.sx = op.sx;
      convt_schedule(t, e.cu_count);
      ws.route[i].geom = t;
      kind(i) = Route::ConvT;
    }
  }

  // 8. convt3 (four consecutive ops from ConvPipe / ConvIgemm): ConvTranspose2d(3, s2, p1, op1) as
  // its phase ops (protonet): one convt3.hip launch from the phase-(0,0) op over the shared input
  // halo; the other three launch nothing
  void pass_convt3() {
    for (size_t i = 0; i + 3 < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if (!e.packed[i].w_ct3 || op.kind != OP_CONV || op.segs.size() != 1 || op.segs[0].convt_phase != 0 ||
          op.up_s != 2 || op.out < 0 || op.add >= 0)
        continue;
      bool ok = true;
      for (int ph = 0; ph < 4; ++ph) {
        const OpSpec& o = plan.ops[i + ph];
        ok = ok && generic(i + ph) && o.kind == OP_CONV && o.segs.size() == 1 && o.segs[0].convt_phase == ph &&
             o.segs[0].src == op.segs[0].src && o.out == op.out && o.up_s == 2 && o.act == op.act && o.add < 0;
      }
      const TensorSpec& src = plan.tensors[op.segs[0].src];
      const TensorSpec& tgt = plan.tensors[op.out];
      ok = ok && tgt.H == 2 * src.H && tgt.W == 2 * src.W && op.N == tgt.C &&
           convt3_supported(src.C, op.N, src.C, tgt.C, src.H, src.W, esz);
      if (!ok) continue;
      ConvT3Params t{};
      t.src = at(op.segs[0].src); t.B = B; t.H = src.H; t.W = src.W; t.C = src.C; t.ldc = src.C;
      t.act = op.act; t.N = op.N;
      t.out = at(op.out); t.out_ldc = tgt.C;
      convt3_tile(t.H, t.W, &t.tw, &t.tr);
      ws.route[i].geom = t;
      kind(i) = Route::ConvT3;
      for (int ph = 1; ph < 4; ++ph) kind(i + ph) = Route::ConvT3Done;
    }
  }

  // 9. conv_lat (from ConvPipe / ConvIgemm / Conv3x3 / Conv3x3S2): layers the chosen kernel spreads
  // over fewer work units than the threshold (the deep pyramid levels: a few 512-pixel tiles on 256
  // CUs) -> conv_lat.hip (small tiles, K split over waves)
  void pass_conv_lat() {
    const int lat_min = e.lat_units >= 0 ? e.lat_units : e.cu_count;
    for (size_t i = 0; e.lat_mode && (dtype != F32 || e.lat_f32) && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      ConvParams& p = ws.params[i];
      const bool c3 = kind(i) == Route::Conv3x3, s2 = kind(i) == Route::Conv3x3S2;
      if (!(generic(i) || c3 || s2) || op.kind != OP_CONV || op.up_s || op.out < 0 || op.out_f32 || op.add >= 0 || !lat_ok[i] ||
          p.N % 8 || p.out_ldc % 8 || p.out_coff % 8)
        continue;
      long units = 0;  // conv_igemm corner case: always worse than conv_lat
      if (c3) {
        const C3Geom& g = std::get<C3Geom>(ws.route[i].geom);
        units = (long)p.mtiles * p.ntiles * (g.ni == 2 && p.N > 64 ? 2 : 1) / (g.nw == 4 ? 2 : 1);
      } else if (s2 || kind(i) == Route::ConvPipe) {
        units = s2 ? p.mtiles : (long)p.mtiles * p.ntiles;
      }
      if (units >= lat_min) continue;
      const int nks = (int)op_ks[i].size();
      if (nks < 2) continue;
      // only when its 64 x 128 tiles fit one round of workgroups (one per CU): measured on MI355X, a
      // second round costs more than the halo kernels' under-filled grid (30x40 level at B=32:
      // 44-50 us vs 24 us), one round wins or ties (15x20 and below, Roots, DLA-34's 27-channel
      // offset / mask conv at 15x20: 43 vs 98 us)
      int lmt = 0, lnt = 0;
      if (e.lat_units < 0 && conv_lat_tiles(p.M, p.N, &lmt, &lnt) > e.cu_count) continue;
      conv_lat_tiles(p.M, p.N, &p.mtiles, &p.ntiles);
      p.nks = nks;
      kind(i) = Route::ConvLat;
    }
  }

  // 10. conv_burst (from ConvLat): the conv_lat layers conv_burst.hip represents (every segment a
  // 3x3 / stride 1 window or a 1x1 over 128-channel multiples, K <= 1280, the staged window within
  // LDS) take the one-shot kernel: no k-step chain, no split-K hand-off (knob TV_BURST=0 keeps them
  // on conv_lat, 2 = every layer it represents)
  void pass_conv_burst() {
    for (size_t i = 0; e.burst_mode && dtype != F32 && i < nops; ++i) {  // (fp16 / bf16 kernel)
      if (kind(i) != Route::ConvLat) continue;
      BurstParams bp{};
      if (!conv_burst_plan(ws.params[i], B, &bp)) continue;
      // only where every tile is resident at once with a small window: measured (profiles/r5): a
      // second round of tiles, or one workgroup per CU for an 89 KiB 80-column window, loses to
      // conv_lat's split-K (60x80 at B=1: 25.6 vs 16.5 us per launch; 15x20 at B=32: 16.7 vs 17 us)
      const int per_cu = std::min(3, (160 * 1024) / std::max(1, bp.lds));
      if (e.burst_mode == 1 && (bp.lds > 64 * 1024 || conv_burst_workgroups(bp) > per_cu * e.cu_count)) continue;
      ws.route[i].geom = bp;
      kind(i) = Route::ConvBurst;
    }
  }

  // 11. conv1x1_stream (from ConvPipe / ConvIgemm): stride-1 1x1 convs over concatenated inputs (the
  // Roots) that the generic GEMM would run: the streaming kernel (conv1x1.hip) with the weights
  // resident in LDS, 128 output channels per workgroup (knob TV_C1X1=0: off, 2: only layers of at
  // most 128 output channels)
  void pass_conv1x1() {
    for (size_t i = 0; e.c1x1_mode && dtype != F32 && i < nops; ++i) {
      const OpSpec& op = plan.ops[i];
      if (!generic(i) || op.kind != OP_CONV || op.up_s || op.add >= 0 || op.out < 0 || op.out_f32) continue;
      bool one = !op.segs.empty();
      for (const SegSpec& sg : op.segs)
        one = one && sg.kh == 1 && sg.kw == 1 && sg.stride == 1 && sg.pad == 0 && !sg.row_expand && sg.convt_phase < 0;
      if (one && conv1x1_stream_supported(ws.params[i], esz) && !(e.c1x1_mode == 2 && ws.params[i].N > 128))
        kind(i) = Route::Conv1x1;
    }
  }

  // conv_lat split-K over workgroups for the layers whose tiles leave most CUs idle (the latency
  // path: at B=1 every conv_lat layer is one k-step chain of ~9 latency-bound k-steps per K group):
  // up to lat_split_max workgroups per tile, each slice >= 2 k-steps (one per K group), the tiles x
  // slices within one round of CUs. Partial tiles meet in `slab`, tickets in `cnt` (conv_lat.hip).
  void split_conv_lat() {
    for (size_t i = 0; i < nops; ++i) {
      if (kind(i) != Route::ConvLat) continue;
      ConvParams& p = ws.params[i];
      const int tiles = p.mtiles * p.ntiles;
      // only layers with a long k-step chain: measured at B=1 (profiles/r5/b1_knobs.txt), the hand-off
      // (write-through partial tiles, ticket, sc1 loads) costs more than it saves on the 18-20 k-step
      // 128-channel layers (R18 1.295 -> 1.269 ms without it) and far less on DLA-34's 36-72 k-step
      // 256 / 512-channel ones (1.284 -> 1.398 ms without it)
      // (fp32: a k-step is a quarter of the fp16 one's MFMA rate at half its depth, so the chains are
      // twice as long and 2x slower per step: up to lat_split_max_f32 slices)
      const int smax = dtype == F32 ? e.lat_split_max_f32 : e.lat_split_max;
      int ks = p.nks >= e.lat_split_min_nks ? std::min(smax, p.nks / 2) : 1;
      ks = std::min(ks, e.cu_count / std::max(1, tiles));
      p.ksplit = ks > 1 ? ks : 0;
      if (!p.ksplit) continue;
      ws.lat_slab_floats = std::max(ws.lat_slab_floats, (size_t)tiles * ks * kLatSlabFloats);
      ws.lat_tickets = std::max(ws.lat_tickets, (size_t)tiles);
    }
    ws.lat_slots = grouping ? kLatGroupMax : 1;
    if (ws.lat_tickets) ws.cnt_bytes = align_up(ws.lat_slots * ws.lat_tickets * sizeof(unsigned), 16);
  }

  // The schedule: in execution order, consecutive ConvBurst / ConvLat / ConvT ops of one level share
  // a launch (up to k*GroupMax; ConvLat and ConvT within one round of CUs). Slot k of a ConvLat
  // group has its own split-K slab and tickets.
  void plan_groups() {
    auto lat_wgs = [&](int i) { const ConvParams& p = ws.params[i]; return p.mtiles * p.ntiles * std::max(1, p.ksplit); };
    auto convt = [&](int i) -> const ConvTParams& { return std::get<ConvTParams>(ws.route[i].geom); };
    // a ConvT + add on convt.hip that covers its whole target (no uncovered-margin copy after it)
    auto convt_groupable = [&](int i) {
      const OpSpec& op = plan.ops[i];
      if (kind(i) != Route::ConvT || op.out < 0) return false;
      const TensorSpec& tg = plan.tensors[op.out];
      return op.cov_y0 <= 0 && op.cov_x0 <= 0 && op.cov_y1 >= tg.H && op.cov_x1 >= tg.W;
    };
    ws.groups.clear();
    for (size_t k = 0; k < nops;) {
      const int i = ws.order[k++];
      std::vector<int> g{i};
      // the next op in execution order, when it is on op i's level and `fits`
      auto take = [&](int max, auto fits) {
        if (k >= nops || (int)g.size() >= max) return false;
        const int j = ws.order[k];
        if (ws.level[j] != ws.level[i] || !fits(j)) return false;
        g.push_back(j);
        ++k;
        return true;
      };
      if (grouping && kind(i) == Route::ConvBurst) {  // one-shot layers of one level: no CU budget (no tickets)
        while (take(kBurstGroupMax, [&](int j) { return kind(j) == Route::ConvBurst; })) {}
      } else if (grouping && kind(i) == Route::ConvLat) {
        int used = lat_wgs(i);
        while (take(kLatGroupMax, [&](int j) { return kind(j) == Route::ConvLat && used + lat_wgs(j) <= e.cu_count; })) {
          ws.route[g.back()].slot = (int)g.size() - 1;
          used += lat_wgs(g.back());
        }
      } else if (grouping && convt_groupable(i)) {  // up-steps of one level with the same phase grouping
        int used = convt_workgroups(convt(i));
        while (take(kConvTGroupMax, [&](int j) {
          return convt_groupable(j) && convt(j).np == convt(i).np && used + convt_workgroups(convt(j)) <= e.cu_count;
        }))
          used += convt_workgroups(convt(g.back()));
      }
      ws.groups.push_back(std::move(g));
    }
  }

  // conv_pipe split-K for layers whose 256 x 128 tiles fill the CUs badly: the fp32 path's
  // deep levels at small batches (R18 at B=1: a 15x20 level is 2 tiles of 36 k-steps on 2 of 256
  // CUs) and its 300-tile 240x320 layers (two rounds, the second 17% full). ksplit workgroups per
  // tile, partial tiles meet in pslab, tickets in pcnt (knob TV_PIPE_SPLIT: 0 off, 1 fp32 only,
  // 2 every dtype; TV_PIPE_SPLIT_MAX slices per tile; TV_PIPE_SPLIT_RED hand-off cost)
  void split_conv_pipe() {
    if (!(e.pipe_split_mode == 2 || (e.pipe_split_mode == 1 && dtype == F32))) return;
    for (size_t i = 0; i < nops; ++i) {
      ConvParams& p = ws.params[i];
      if (kind(i) != Route::ConvPipe) continue;  // (both epilogues: the ConvT phase scatter + add runs after the sum)
      // slices per tile by a cost model in tenths of a k-step: rounds of workgroups x k-steps per
      // slice, plus the hand-off (each slice's partial tile written, then read by the reducer:
      // pipe_split_red per slice); split only when it saves >= 10%
      const long tiles = (long)p.mtiles * p.ntiles;
      auto cost = [&](int k) {
        const long rounds = (tiles * k + e.cu_count - 1) / e.cu_count;
        return rounds * ((p.nks + k - 1) / k) * 10 + (k > 1 ? (long)e.pipe_split_red * (k + 1) : 0);
      };
      int ks = 1;
      for (int k = 2; k <= e.pipe_split_max && k <= p.nks / 2; ++k)
        if (cost(k) < cost(ks)) ks = k;
      if (cost(ks) * 10 > cost(1) * 9) ks = 1;
      p.ksplit = ks > 1 ? ks : 0;
      if (!p.ksplit) continue;
      ws.pipe_slab_floats = std::max(ws.pipe_slab_floats, (size_t)tiles * ks * kPipeTileM * 128);
      ws.pipe_tickets = std::max(ws.pipe_tickets, (size_t)tiles);
    }
  }

  // the k-step descriptor lists of the ops that ended on a kernel that walks them
  void collect_ksteps() {
    ws.ks_off.assign(nops, 0);
    for (size_t i = 0; i < nops; ++i) {
      if (kind(i) != Route::ConvPipe && kind(i) != Route::ConvLat) continue;
      ws.ks_off[i] = ws.ksteps.size();
      ws.ksteps.insert(ws.ksteps.end(), op_ks[i].begin(), op_ks[i].end());
    }
  }

  void run() {
    ws.B = B, ws.kname.assign(nops, std::string());
    plan_levels(); fixed_routes(); pass_stem_pool(); plan_arena(); conv_geometry();
    // the kernel choice: each pass may only take an op from the routes its comment names
    pass_generic(); pass_conv3x3(); pass_conv3x3s2(); pass_conv_small(); pass_dcn(); pass_heads();
    pass_convt(); pass_convt3(); pass_conv_lat(); pass_conv_burst(); pass_conv1x1();
    split_conv_lat(); plan_groups(); split_conv_pipe(); collect_ksteps();
  }
};

}  // namespace

void Engine::plan_schedule(int B, Workspace* ws) const { Planner{*this, B, *ws}.run(); }

}  // namespace tv
