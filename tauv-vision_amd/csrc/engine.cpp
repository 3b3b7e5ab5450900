// Engine: create (configure on the host, then upload the host-packed weights of pack.cpp),
// liveness-planned HBM workspace per (stream, batch), and the launch sequence of one forward.
// C ABI in capi.cpp.
#include "engine.h"

#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <memory>

namespace tv {

// Op i's weights: packed on the host (pack.cpp), uploaded, and the host copy released.
int Engine::pack_op(size_t oi) {
  HostPacked hp;
  int rc = pack_op_host(plan, oi, dtype, host_w, stem_op, ct3_mode, &hp);
  if (rc) return rc;
  Packed& pk = packed[oi];
  pk.Npad = hp.Npad;
  pk.Kpad = hp.Kpad;
  pk.seg_ksteps = hp.seg_ksteps;
  std::copy(hp.head_row0, hp.head_row0 + 16, pk.head_row0);
  std::copy(hp.head_nrows, hp.head_nrows + 16, pk.head_nrows);
  pk.head_ok = !hp.head_w.empty();
  auto upload = [](auto*& dst, const auto& src) {
    if (src.empty()) return (int)TV_OK;
    const size_t bytes = src.size() * sizeof(src[0]);
    TV_HIP(hipMalloc((void**)&dst, bytes));
    TV_HIP(hipMemcpy(dst, src.data(), bytes, hipMemcpyHostToDevice));
    return (int)TV_OK;
  };
  if ((rc = upload(pk.w_ct3, hp.w_ct3)) || (rc = upload(pk.head_w, hp.head_w)) || (rc = upload(pk.head_b, hp.head_b)) ||
      (rc = upload(pk.w, hp.w)) || (rc = upload(pk.bias, hp.bias)))
    return rc;
  weight_bytes += hp.w_ct3.size() + hp.w.size() + hp.bias.size() * 4;
  return TV_OK;
}

// Every decision of create, on the host (no HIP call): the plan, the diagnostic knobs, and the
// fusions that decide how an op's weights are packed. `cus` = the device's compute units.
int Engine::configure(const tv_model_desc& d, const std::vector<std::pair<std::string, std::string>>& knobs, int cus) {
  desc = d;
  cu_count = cus;
  if (desc.compute_dtype == TV_F32X3) {  // fp32 storage; the pipelined GEMMs' products as three fp16 MFMAs
    desc.compute_dtype = TV_F32;
    f32x3 = 1;
  }
  dtype = desc.compute_dtype;
  int rc = build_plan(desc, &plan);
  if (rc) return rc;
  // diagnostics only (tv_engine_create_diag): kernel-choice overrides for A/B experiments; the
  // product entry point (tv_engine_create) passes none and reads no environment
  for (const auto& kv : knobs) {
    const std::string& k = kv.first;
    const char* env = kv.second.c_str();
    const int v = std::atoi(env);
    if (k == "TV_CONV_PIPE") pipe_mode = v;
    else if (k == "TV_CONV3") conv3_mode = v;
    else if (k == "TV_C3_TW") c3_tw_force = v == 16 ? 16 : v == 32 ? 32 : 0;
    else if (k == "TV_CUS") cu_count = std::max(8, std::min(cu_count, v));
    else if (k == "TV_STEM") stem_mode = v;
    else if (k == "TV_STEMFUSE") stemfuse_mode = v;
    else if (k == "TV_RSTEM") rstem_mode = v;
    else if (k == "TV_LAT") lat_mode = v;
    else if (k == "TV_LAT_UNITS") lat_units = v;
    else if (k == "TV_LAT_SPLIT") lat_split_max = std::max(1, std::min(8, v));
    else if (k == "TV_LAT_SPLIT_MIN") lat_split_min_nks = std::max(0, v);
    else if (k == "TV_LAT_F32") lat_f32 = v ? 1 : 0;
    else if (k == "TV_LAT_SPLIT_F32") lat_split_max_f32 = std::max(1, std::min(16, v));
    else if (k == "TV_PIPE_SPLIT") pipe_split_mode = std::max(0, std::min(2, v));
    else if (k == "TV_PIPE_SPLIT_MAX") pipe_split_max = std::max(1, std::min(64, v));
    else if (k == "TV_PIPE_SPLIT_RED") pipe_split_red = std::max(0, v);
    else if (k == "TV_F32X3") f32x3 = v ? 1 : 0;
    else if (k == "TV_LATGROUP") lat_group = v ? 1 : 0;
    else if (k == "TV_CT3") ct3_mode = v ? 1 : 0;
    else if (k == "TV_BURST") burst_mode = std::max(0, std::min(2, v));
    else if (k == "TV_C1X1") c1x1_mode = std::max(0, std::min(2, v));
    else if (k == "TV_LATGROUP_B") lat_group_max_b = std::max(1, v);
    else if (k == "TV_DCN64") dcn64_mode = v;
    else if (k == "TV_DCN_SPLIT") dcn_split_max = std::max(0, std::min(9, v));
    else if (k == "TV_CONVT") convt_mode = v;
    else if (k == "TV_CONV3S2") s2_mode = v;
    else if (k == "TV_CONV3_MINPIX") conv3_min_pix = v;
    else if (k == "TV_HEADFUSE") headfuse_mode = v;
    else if (k == "TV_S2_MINTILES") s2_min_tiles = v;
    else if (k == "TV_C3_NI") c3_ni_force = v == 2 ? 2 : v == 4 ? 4 : 0;
    else if (k == "TV_C3_NW") c3_nw_mode = v == 8 ? 8 : 0;
    else if (k == "TV_C3_HALF_COST") c3_half_cost = v;
    else if (k == "TV_CSM_HALO") csm_halo = std::max(0, std::min(2, v));
    else if (k == "TV_SLICES") slices = std::max(1, std::min(kMaxSlices, v));
    else if (k == "TV_SLICE_LAG") slice_lag = std::max(0, v);
    else if (k == "TV_C3_STAMPS") {  // "op:device pointer" (stamp builds of conv3x3 only; create checks the pointer)
#if defined(TV_C3_EXP) && TV_C3_EXP == 9
      stamp_op = v;
      const char* c = std::strchr(env, ':');
      stamp_buf = c ? reinterpret_cast<unsigned long long*>(std::strtoull(c + 1, nullptr, 0)) : nullptr;
#else
      set_error("TV_C3_STAMPS needs the stamp build of the library (EXTRA=-DTV_C3_EXP=9)");
      return TV_EINVAL;
#endif
    }
    else if (k == "TV_SLICE_SIZES") {
      for (const char* c = env; *c;) {
        slice_sizes_env.push_back(std::atoi(c));
        while (*c && *c != ',') ++c;
        if (*c == ',') ++c;
      }
    } else {
      set_error("unknown engine knob: " + k);
      return TV_EINVAL;
    }
  }
  // fused staging + stem (stem.hip): the row-expanded 7x7 conv right after the staging op
  if (stem_mode && dtype != F32)
    for (size_t i = 0; i + 1 < plan.ops.size(); ++i)
      if (plan.ops[i].kind == OP_PREP && plan.ops[i + 1].kind == OP_CONV && plan.ops[i + 1].segs.size() == 1 &&
          plan.ops[i + 1].segs[0].row_expand == 7 && plan.ops[i + 1].N <= 128 && plan.ops[i + 1].N % 8 == 0 &&
          plan.ops[i + 1].act == 1 && plan.ops[i + 1].segs[0].stride == 1) {  // (ResNet's stride-2 stem: the generic GEMMs)
        stem_op = (int)i + 1;
        break;
      }
  // stem + block0.conv1 in one launch (stem_s2.hip): the 128-channel stem feeds exactly the block's
  // stride-2 3x3 conv1 and its stride-2 1x1 conv_residual (dla.py:13-37, 182-186). The plan gets a
  // tensor R = stem(2y, 2x) [Ho, Wo, 128], written by the fused launch (conv1's second output) and
  // read by conv2's residual segment at stride 1; the stem output itself is never stored.
  if (stemfuse_mode && stem_op >= 0 && stem_op + 2 < (int)plan.ops.size()) {
    const OpSpec& st = plan.ops[stem_op];
    const OpSpec& c1 = plan.ops[stem_op + 1];
    const OpSpec& c2 = plan.ops[stem_op + 2];
    const int so = st.out;
    bool ok = st.N == 128 && so >= 0 && plan.tensors[so].C == 128 && c1.kind == OP_CONV && c1.segs.size() == 1 &&
              c1.segs[0].src == so && c1.segs[0].kh == 3 && c1.segs[0].kw == 3 && c1.segs[0].stride == 2 &&
              c1.segs[0].pad == 1 && (c1.segs[0].pad_w < 0 || c1.segs[0].pad_w == 1) && !c1.segs[0].row_expand &&
              c1.segs[0].ci0 == 0 && c1.segs[0].cin == 128 && c1.N == 128 && c1.act == 1 && c1.out >= 0 &&
              c1.add < 0 && !c1.up_s && c1.stack_w.empty() && plan.tensors[c1.out].C == 128 &&
              plan.tensors[c1.out].H == (desc.in_h + 1) / 2 && plan.tensors[c1.out].W == (desc.in_w + 1) / 2 &&
              c2.kind == OP_CONV && c2.segs.size() == 2 && c2.segs[0].src == c1.out && c2.segs[1].src == so &&
              c2.segs[1].kh == 1 && c2.segs[1].kw == 1 && c2.segs[1].stride == 2 && c2.segs[1].pad == 0 &&
              !c2.segs[1].identity && c2.segs[1].ci0 == 0 && c2.segs[1].cin == 128;
    for (size_t i = 0; ok && i < plan.ops.size(); ++i) {  // nothing else reads the stem output
      if ((int)i == stem_op + 1 || (int)i == stem_op + 2) continue;
      const OpSpec& o = plan.ops[i];
      ok = o.src != so && o.add != so;
      for (const SegSpec& sg : o.segs) ok = ok && sg.src != so;
    }
    if (ok) {
      const TensorSpec t1 = plan.tensors[c1.out];
      plan.tensors.push_back(TensorSpec{t1.H, t1.W, 128});
      const int r = (int)plan.tensors.size() - 1;
      plan.ops[stem_op + 1].out2 = r;
      plan.ops[stem_op + 2].segs[1].src = r;
      plan.ops[stem_op + 2].segs[1].stride = 1;
      ss2_op = stem_op + 1;
    }
  }
  // ResNet-18's stem (resnet.hip stem7s2_pool): staging, the stride-2 row-expanded 7x7 conv 3 -> 64 with
  // ReLU and the 3x3 / s2 max-pool of its output, which nothing else reads
  if (rstem_mode && dtype != F32)
    for (size_t i = 0; i + 2 < plan.ops.size(); ++i) {
      const OpSpec& st = plan.ops[i + 1];
      const OpSpec& mp = plan.ops[i + 2];
      if (plan.ops[i].kind != OP_PREP || st.kind != OP_CONV || st.segs.size() != 1 || st.segs[0].row_expand != 7 ||
          st.segs[0].stride != 2 || st.segs[0].src != plan.ops[i].out || st.segs[0].cin != 3 || st.N != 64 ||
          st.act != 1 || st.out < 0 || mp.kind != OP_MAXPOOL3S2 || mp.src != st.out)
        continue;
      bool ok = true;
      for (size_t j = 0; ok && j < plan.ops.size(); ++j) {
        if (j == i + 2) continue;
        const OpSpec& o = plan.ops[j];
        ok = o.src != st.out && o.add != st.out;
        for (const SegSpec& sg : o.segs) ok = ok && sg.src != st.out;
      }
      if (ok) rstem_op = (int)i + 1;
      break;
    }
  return TV_OK;
}

// The caller's weight views by name (valid during create only)
int weight_views(const tv_weight_view* w, int n, HostWeights* host_w) {
  for (int i = 0; i < n; ++i) {
    if (!w[i].name || (!w[i].data && w[i].numel)) {
      set_error("null weight view");
      return TV_EINVAL;
    }
    (*host_w)[w[i].name] = {w[i].data, w[i].numel};
  }
  return TV_OK;
}

int Engine::create(const tv_model_desc& d, const tv_weight_view* w, int n, int dev,
                   const std::vector<std::pair<std::string, std::string>>& knobs) {
  device = dev;
  int rc = weight_views(w, n, &host_w);
  if (rc) return rc;
  TV_HIP(hipSetDevice(device));
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = cu_count;
  rc = configure(d, knobs, ncu);
  if (rc) return rc;
#if defined(TV_C3_EXP) && TV_C3_EXP == 9
  for (const auto& kv : knobs) {
    if (kv.first != "TV_C3_STAMPS") continue;
    // the stamp kernel writes 8 counters per wave of every workgroup it may launch (<= one per
    // CU, 8 waves): the pointer must lie in a device allocation with that much room after it
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    const size_t need = (size_t)cu_count * 8 * 8 * sizeof(unsigned long long);
    if (!stamp_buf || hipMemGetAddressRange(&base, &size, stamp_buf) != hipSuccess ||
        (char*)stamp_buf + need > (char*)base + size) {
      (void)hipGetLastError();
      set_error("TV_C3_STAMPS: the pointer is not inside a device allocation of >= " + std::to_string(need) +
                " bytes");
      return TV_EINVAL;
    }
  }
#endif
  TV_HIP(hipMalloc(&zero_page, 256));
  TV_HIP(hipMemset(zero_page, 0, 256));
  packed.resize(plan.ops.size());
  for (size_t i = 0; i < plan.ops.size(); ++i) {
    rc = pack_op(i);
    if (rc) return rc;
  }
  host_w.clear();  // views are only valid during create
  return TV_OK;
}

Engine::~Engine() {
  if (zero_page) (void)hipFree(zero_page);
  for (auto& p : packed)
    for (void* q : {p.w, p.w_c3, p.w_c3h, p.w_c3e, p.w_ss2, p.w_burst, p.w_x3, p.w_ct3, p.head_w, (void*)p.head_b,
                    (void*)p.bias})
      if (q) (void)hipFree(q);
  for (auto& kv : workspaces) delete kv.second;
  for (auto& kv : side) {
    if (kv.second.fork) (void)hipEventDestroy(kv.second.fork);
    for (hipEvent_t e : kv.second.join) (void)hipEventDestroy(e);
    for (hipStream_t t : kv.second.s) (void)hipStreamDestroy(t);
  }
}

Workspace::~Workspace() {
  for (void* p : {arena, (void*)dparams, (void*)dks, (void*)slab, (void*)cnt, (void*)pslab, (void*)pcnt, (void*)dslab,
                  (void*)dcnt})
    if (p) (void)hipFree(p);
  for (hipEvent_t ev : gev) (void)hipEventDestroy(ev);
}

namespace {

// a planned pointer (kArenaTag + offset; null = no tensor) -> its address in the arena
template <class T>
void bind(T*& p, char* arena) {
  if (p) p = (T*)(arena + (reinterpret_cast<uintptr_t>(p) - kArenaTag));
}

// A weight copy in a kernel's own order, made on first use and shared by the workspaces of every
// batch size; `repack(copy)` fills it on the null stream and the device is synchronised after it.
template <class F>
int repacked(void*& copy, size_t bytes, F repack) {
  if (copy) return TV_OK;
  TV_HIP(hipMalloc(&copy, bytes));
  int rc = repack(copy);
  if (rc) return rc;
  TV_HIP(hipDeviceSynchronize());
  return TV_OK;
}

// split-K hand-off buffers: fp32 partial tiles, and tickets zeroed once (the last slice of a tile resets its own)
int alloc_split(float*& slab, size_t floats, unsigned*& cnt, size_t cnt_bytes) {
  if (!cnt_bytes) return TV_OK;
  TV_HIP(hipMalloc((void**)&slab, floats * sizeof(float)));
  TV_HIP(hipMalloc((void**)&cnt, cnt_bytes));
  TV_HIP(hipMemset(cnt, 0, cnt_bytes));
  return TV_OK;
}

}  // namespace

// Op i of a planned workspace: bind its arena pointers, make (once) the weight copy its route
// reads, and patch the weight / bias / hand-off pointers into its launch parameters.
int Engine::bind_op(size_t i, Workspace* ws) {
  const OpSpec& op = plan.ops[i];
  const int esz = dtype_size(dtype);
  char* a = (char*)ws->arena;
  ConvParams& p = ws->params[i];
  Packed& pk = packed[i];
  OpRoute& r = ws->route[i];
  if (op.kind == OP_CONV || op.kind == OP_CONVT_ADD) {
    for (int s = 0; s < p.nseg; ++s) bind(p.seg[s].src, a);
    bind(p.out, a); bind(p.add, a);
    p.weight = pk.w; p.bias = pk.bias; p.zero = zero_page;
  }
  switch (r.kind) {
    case Route::StemS2:  // block0.conv1 fused with the stem: its weights in stem_s2.hip's k-step order
      return repacked(pk.w_ss2, stem_s2_weight_bytes(), [&](void* w) { return stem_s2_repack(pk.w, pk.Kpad, esz, w, nullptr); });
    case Route::Conv3x3:
    case Route::HeadsFused: {
      const C3Geom& g = std::get<C3Geom>(r.geom);
      const int epi = r.kind == Route::HeadsFused, ncb = p.seg[0].C / 32;
      const int k16 = conv3x3_k16(epi, g.res, g.ni, g.nw);
      // (the fused-heads body may read another swizzle than the plain 128-channel-tile body: its own copy then)
      void*& wc = g.ni != 4 ? pk.w_c3h : epi && k16 != conv3x3_k16(0, 0, 4, 8) ? pk.w_c3e : pk.w_c3;
      int rc = repacked(wc, conv3x3_weight_bytes(p.ntiles, g.res, ncb), [&](void* w) {
        return conv3x3_repack(pk.w, pk.Kpad, esz, p.ntiles, g.res, g.ni, ncb, k16, w, nullptr);
      });
      if (rc) return rc;
      p.weight = wc;
      if (epi) p.head_w = packed[i + 1].head_w, p.head_b = packed[i + 1].head_b;
      if (stamp_op == (int)i) p.dbg = stamp_buf;
      return TV_OK;
    }
    case Route::Conv3x3S2: {
      int rc = repacked(pk.w_c3, conv3x3s2_weight_bytes(), [&](void* w) { return conv3x3s2_repack(pk.w, pk.Kpad, esz, w, nullptr); });
      p.weight = pk.w_c3;
      return rc;
    }
    case Route::ConvBurst: {
      BurstParams& bp = std::get<BurstParams>(r.geom);
      int rc = repacked(pk.w_burst, conv_burst_weight_bytes(bp), [&](void* w) { return conv_burst_repack(pk.w, pk.Kpad, esz, bp, w, nullptr); });
      for (int s = 0; s < bp.nseg; ++s) bind(bp.seg[s].src, a);
      bind(bp.out, a);
      bp.w = pk.w_burst; bp.bias = pk.bias;
      return rc;
    }
    case Route::ConvPipe:
    case Route::ConvLat: {
      const bool lat = r.kind == Route::ConvLat;
      p.ks = ws->dks + ws->ks_off[i];
      if (p.ksplit) {  // conv_lat: the region of its slot in a grouped launch
        p.slab = lat ? ws->slab + (size_t)r.slot * ws->lat_slab_floats : ws->pslab;
        p.cnt = lat ? ws->cnt + (size_t)r.slot * ws->lat_tickets : ws->pcnt;
      }
      if (dtype != F32 || !f32x3) return TV_OK;
      // fp32 X3: the pipelined and conv_lat layers read the hi / lo fp16 copy of their weights
      int rc = repacked(pk.w_x3, (size_t)pk.Npad * pk.Kpad * 4, [&](void* w) { return conv_pipe_x3_repack(pk.w, pk.Npad, pk.Kpad, w, nullptr); });
      p.weight = pk.w_x3;
      return rc;
    }
    case Route::DcnFused: {
      DcnParams& q = std::get<DcnParams>(r.geom);
      bind(q.x, a); bind(q.om, a); bind(q.out, a);
      q.w = pk.w; q.bias = pk.bias;
      if (q.ksplit > 1) q.slab = ws->dslab, q.cnt = ws->dcnt;
      return TV_OK;
    }
    case Route::ConvT: {
      ConvTParams& t = std::get<ConvTParams>(r.geom);
      bind(t.src, a); bind(t.add, a); bind(t.out, a);
      t.weight = pk.w; t.bias = pk.bias;
      return TV_OK;
    }
    case Route::ConvT3: {
      ConvT3Params& t = std::get<ConvT3Params>(r.geom);
      bind(t.src, a); bind(t.out, a);
      t.w = pk.w_ct3; t.bias = pk.bias;
      return TV_OK;
    }
    default:
      return TV_OK;
  }
}

// The device side of a planned workspace: the arena, the split-K hand-off buffers (tickets zeroed
// once), the k-step descriptors, each op's pointers and weight copy, the parameter upload.
int Engine::materialize(Workspace* ws) {
  TV_HIP(hipSetDevice(device));
  TV_HIP(hipMalloc(&ws->arena, std::max<size_t>(ws->bytes, 256)));
  int rc = alloc_split(ws->slab, ws->lat_slots * ws->lat_slab_floats, ws->cnt, ws->cnt_bytes);
  if (!rc) rc = alloc_split(ws->pslab, ws->pipe_slab_floats, ws->pcnt, ws->pipe_tickets * sizeof(unsigned));
  if (!rc) rc = alloc_split(ws->dslab, ws->dcn_slab_floats, ws->dcnt, ws->dcn_tickets * sizeof(unsigned));
  if (rc) return rc;
  if (!ws->ksteps.empty()) {
    for (KStep& d : ws->ksteps) bind(d.src, (char*)ws->arena);
    TV_HIP(hipMalloc((void**)&ws->dks, ws->ksteps.size() * sizeof(KStep)));
    TV_HIP(hipMemcpy(ws->dks, ws->ksteps.data(), ws->ksteps.size() * sizeof(KStep), hipMemcpyHostToDevice));
  }
  for (size_t i = 0; !rc && i < plan.ops.size(); ++i) rc = bind_op(i, ws);
  if (rc) return rc;
  TV_HIP(hipMalloc((void**)&ws->dparams, ws->params.size() * sizeof(ConvParams)));
  TV_HIP(hipMemcpy(ws->dparams, ws->params.data(), ws->params.size() * sizeof(ConvParams), hipMemcpyHostToDevice));
  return TV_OK;
}

int Engine::get_workspace(int B, hipStream_t stream, Workspace** out) {
  std::lock_guard<std::mutex> g(mu);
  auto key = std::make_pair((void*)stream, B);
  auto it = workspaces.find(key);
  if (it != workspaces.end()) {
    *out = it->second;
    return TV_OK;
  }
  auto ws = std::make_unique<Workspace>();  // (freed with everything it holds if materialize fails)
  plan_schedule(B, ws.get());
  int rc = materialize(ws.get());
  if (rc) return rc;
  *out = workspaces[key] = ws.release();
  return TV_OK;
}

int Engine::trim() {
  std::lock_guard<std::mutex> g(mu);
  TV_HIP(hipSetDevice(device));
  TV_HIP(hipDeviceSynchronize());  // no queued launch still reads an arena
  for (auto& kv : workspaces) delete kv.second;
  workspaces.clear();
  return TV_OK;
}

int Engine::run_op(size_t i, Workspace* ws, const IoPtrs& io, int input_u8, hipStream_t s) {
  const OpSpec& op = plan.ops[i];
  const OpRoute& r = ws->route[i];
  char* base = (char*)ws->arena;
  const ConvParams* dp = ws->dparams + i;
  const bool out_f32 = op.out < 0 || op.out_f32, x3 = dtype == F32 && f32x3;
  const int mode = op.kind == OP_CONVT_ADD || op.up_s ? 1 : 0;
  // the caller's buffers this op touches: input op.io (staging / layout ops), output -1 - op.out
  // (the fused heads launch writes the output of the 1x1 heads' op, the next one)
  const void* input = io.in[op.io];
  const int oslot = r.kind == Route::HeadsFused ? plan.ops[i + 1].out : op.out;
  float* out = oslot < 0 ? io.out[-1 - oslot] : nullptr;
  const IoSpec ospec = oslot < 0 ? plan.outspec(oslot) : IoSpec{};
  const size_t out_floats = (size_t)ws->B * ospec.H * ospec.W * ospec.cpad;
  int rc = TV_OK;
  switch (r.kind) {
    case Route::StagingInStem:  // staging runs inside the stem kernel
    case Route::StemInS2:       // the stem runs inside block0.conv1's launch
    case Route::DcnInFused:     // sampled inside the next op's fused DCNv2 kernel
    case Route::ConvT3Done:     // a ConvTranspose2d phase done by the phase-(0,0) op's launch
    case Route::StemInPool:     // the stem runs inside the max-pool op's launch
      return TV_OK;
    case Route::StemPool: {
      const Packed& pk = packed[rstem_op];
      // (u8 NHWC camera frames: the kernel's LUT instance, ToTensor + Normalize as launch_prep_u8's)
      const StemPoolParams sp{io.in[plan.ops[rstem_op - 1].io], pk.w, pk.bias, base + ws->off[op.out],
                              ws->B, desc.in_h, desc.in_w, pk.Kpad, input_u8 ? 1 : 0};
      return launch_stem7s2_pool(sp, dtype, cu_count, s);
    }
    case Route::Staging: {
      void* dst = base + ws->off[op.out];
      return input_u8 ? launch_prep_u8((const uint8_t*)input, ws->B, desc.in_h, desc.in_w, dst, plan.in_cpad, dtype, s)
                      : launch_prep_nchw((const float*)input, ws->B, desc.in_h, desc.in_w, dst, plan.in_cpad, dtype, s);
    }
    case Route::StemS2: {
      const TensorSpec& t1 = plan.tensors[op.out];
      StemS2Params sp{};
      sp.input = input; sp.u8 = input_u8;
      sp.B = ws->B; sp.H = desc.in_h; sp.W = desc.in_w; sp.Ho = t1.H; sp.Wo = t1.W;
      sp.stem_w = packed[stem_op].w; sp.stem_bias = packed[stem_op].bias;
      sp.w1 = packed[i].w_ss2; sp.bias1 = packed[i].bias;
      sp.out = base + ws->off[op.out]; sp.out_ldc = t1.C;
      sp.res = base + ws->off[op.out2]; sp.res_ldc = plan.tensors[op.out2].C;
      if (stamp_op == (int)i) sp.dbg = stamp_buf;
      return launch_stem_s2(sp, dtype, cu_count, s);
    }
    case Route::Stem: {
      StemParams sp{};
      sp.input = input; sp.u8 = input_u8;
      sp.B = ws->B; sp.H = desc.in_h; sp.W = desc.in_w;
      sp.out = base + ws->off[op.out]; sp.out_ldc = plan.tensors[op.out].C; sp.N = op.N;
      sp.weight = packed[i].w; sp.bias = packed[i].bias;
      return launch_stem(sp, dtype, cu_count, s);
    }
    case Route::LayoutIn:
      if (input_u8) {
        set_error("this model takes an fp32 NCHW feature map, not u8 frames");
        return TV_EINVAL;
      }
      return launch_nchw_to_nhwc((const float*)input, ws->B, op.N, plan.ins[op.io].H, plan.ins[op.io].W,
                                 base + ws->off[op.out], plan.tensors[op.out].C, dtype, s);
    case Route::BilinearAdd: {
      const TensorSpec& src = plan.tensors[op.src];
      const TensorSpec& dst = plan.tensors[op.out];
      return launch_bilinear_add(base + ws->off[op.src], ws->B, src.H, src.W, src.C, base + ws->off[op.out], dst.H,
                                 dst.W, dst.C, op.N, dtype, s);
    }
    case Route::HeadScatter: {
      HeadScatterParams hp{};
      hp.nparts = (int)op.parts.size();
      hp.B = ws->B;
      for (int k = 0; k < hp.nparts; ++k) {
        const ScatterPart& q = op.parts[k];
        const TensorSpec& t = plan.tensors[q.src];
        const long long frame = (long long)plan.outs[q.slot].H * q.width;
        hp.HW = t.H * t.W;
        hp.part[k] = HeadScatterPart{(const float*)(base + ws->off[q.src]), io.out[q.slot] + (size_t)q.row0 * q.width,
                                     frame, t.C, q.c0, q.n, q.tanh ? 1 : 0};
      }
      return launch_head_scatter(hp, s);
    }
    case Route::MaxPool3S2: {
      const TensorSpec& src = plan.tensors[op.src];
      return launch_maxpool3x3s2(base + ws->off[op.src], ws->B, src.H, src.W, src.C, base + ws->off[op.out], dtype, s);
    }
    case Route::AddRelu: {
      const TensorSpec& t = plan.tensors[op.out];
      return launch_add_relu(base + ws->off[op.src], base + ws->off[op.add], base + ws->off[op.out],
                             (long long)ws->B * t.H * t.W * t.C, dtype, s);
    }
    case Route::StoreF32: {
      const TensorSpec& t = plan.tensors[op.src];
      return launch_store_f32(base + ws->off[op.src], out, (long long)ws->B * t.H * t.W * t.C, dtype, s);
    }
    case Route::MaxPool:
    case Route::DcnSample:
    case Route::DwConvTAdd: {
      const TensorSpec& src = plan.tensors[op.src];
      const TensorSpec& dst = plan.tensors[op.out];
      void* o = base + ws->off[op.out];
      const void* x = base + ws->off[op.src];
      if (r.kind == Route::MaxPool) return launch_maxpool2(x, ws->B, src.H, src.W, src.C, o, dst.H, dst.W, dtype, s);
      const TensorSpec& ad = plan.tensors[op.add];
      const void* a = base + ws->off[op.add];
      if (r.kind == Route::DcnSample) return launch_dcn_sample(x, ws->B, src.H, src.W, src.C, a, ad.C, o, dtype, s);
      return launch_dwconvt_add(x, ws->B, src.H, src.W, src.C, (const float*)packed[i].w, op.up_s, a, ad.C, o, dst.H,
                                dst.W, op.sy, op.sx, dtype, s);
    }
    case Route::DcnFused:
      return launch_dcn_gemm(std::get<DcnParams>(r.geom), dtype, dcn64_mode, cu_count, s);
    case Route::HeadsDone:  // fused into the 3x3 heads launch; an activation after the summed 1x1 runs here
      return op.act == 2 ? launch_leaky_inplace(out, out_floats, s) : TV_OK;
    case Route::HeadsFused: {
      const C3Geom& g = std::get<C3Geom>(r.geom);
      if (!ws->params[i].head_store && (rc = launch_fill_zero(out, out_floats * sizeof(float), s))) return rc;
      return launch_conv3x3(ws->params[i], dp, out, dtype, g.tw, g.grid, s, 1);
    }
    case Route::ConvT3:
      return launch_convt3(std::get<ConvT3Params>(r.geom), dtype, cu_count, s);
    case Route::ConvSmall:
      return launch_conv_small(ws->params[i], dp, dtype, cu_count, csm_variant(ws->params[i].seg[0].stride), s);
    case Route::ConvBurst: {
      const BurstParams* bp = &std::get<BurstParams>(r.geom);
      return launch_conv_burst(&bp, 1, dtype, s);
    }
    case Route::ConvLat:
      return launch_conv_lat(ws->params[i], dp, dtype, s, x3);
    case Route::Conv1x1:
      return launch_conv1x1_stream(ws->params[i], dp, dtype, cu_count, s);
    case Route::Conv3x3S2:
      return launch_conv3x3s2(ws->params[i], dp, ws->params[i].out, dtype, std::get<S2Geom>(r.geom).grid, s);
    case Route::Conv3x3: {
      const C3Geom& g = std::get<C3Geom>(r.geom);
      return launch_conv3x3(ws->params[i], dp, ws->params[i].out, dtype, g.tw, g.grid, s, 0, g.res, g.ni, g.nw);
    }
    // the routes an OP_CONVT_ADD can have: the uncovered margin of its target is copied after them
    case Route::ConvT:
      rc = launch_convt(std::get<ConvTParams>(r.geom), dtype, s);
      break;
    case Route::ConvPipe:
    case Route::ConvIgemm: {
      ConvParams p = ws->params[i];
      if (op.out < 0) p.out = out;  // the caller's fp32 output (only these two routes may write it directly)
      rc = r.kind == Route::ConvPipe ? launch_conv_pipe(p, dp, p.out, dtype, out_f32, mode, s, x3)
                                     : launch_conv(p, dp, p.out, dtype, out_f32, mode, s);
      break;
    }
  }
  if (rc || op.kind != OP_CONVT_ADD) return rc;
  const TensorSpec& tgt = plan.tensors[op.out];
  if (op.cov_y0 > 0 || op.cov_x0 > 0 || op.cov_y1 < tgt.H || op.cov_x1 < tgt.W)
    return launch_uncovered_copy(base + ws->off[op.add], plan.tensors[op.add].C, base + ws->off[op.out], tgt.C, tgt.C,
                                 ws->B, tgt.H, tgt.W, op.cov_y0, op.cov_y1, op.cov_x0, op.cov_x1, dtype, s);
  return TV_OK;
}

int Engine::get_side(hipStream_t s, int n, SideStreams** out) {
  std::lock_guard<std::mutex> g(mu);
  SideStreams& ss = side[(void*)s];
  if (!ss.fork) TV_HIP(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
  while ((int)ss.s.size() < n) {
    hipStream_t t;
    hipEvent_t e;
    TV_HIP(hipStreamCreateWithFlags(&t, hipStreamNonBlocking));
    TV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ss.s.push_back(t);
    ss.join.push_back(e);
  }
  *out = &ss;
  return TV_OK;
}

std::vector<int> Engine::slice_sizes(int B) const {
  if (!slice_sizes_env.empty()) {
    int sum = 0;
    for (int v : slice_sizes_env) sum += v > 0 ? v : 1 << 30;
    if (sum == B && (int)slice_sizes_env.size() <= kMaxSlices) return slice_sizes_env;
  }
  if (slices > 1 && B >= slices * slice_min) {
    std::vector<int> sz(slices);
    for (int k = 0; k < slices; ++k) sz[k] = B / slices + (k < B % slices ? 1 : 0);
    return sz;
  }
  return {B};
}

int Engine::run_all(const IoPtrs& io, int input_u8, int B, hipStream_t s, size_t op0, size_t op1) {
  Workspace* ws = nullptr;
  int rc = get_workspace(B, s, &ws);
  if (rc) return rc;
  // conv_lat split-K tickets: zeroed when the workspace is made, and every tile's last-arriving
  // slice resets its own ticket, so each complete forward leaves them all at zero for the next
  // (no per-forward reset launch on the latency path; a memset node in a captured graph also broke
  // the replays after the first on this ROCm: aux.hip fill_zero16)
  const size_t nops = plan.ops.size();
  if (op0 == 0 && op1 >= nops) {  // the whole forward: the schedule's groups
    if (insitu && ws->gev.size() != ws->groups.size() + 1) {
      for (hipEvent_t e : ws->gev) (void)hipEventDestroy(e);
      ws->gev.assign(ws->groups.size() + 1, nullptr);
      for (hipEvent_t& e : ws->gev) TV_HIP(hipEventCreate(&e));
    }
    size_t gi = 0;
    for (const std::vector<int>& g : ws->groups) {
      if (insitu) TV_HIP(hipEventRecord(ws->gev[gi], s));
      ++gi;
      const Route kind = ws->route[g[0]].kind;
      if (g.size() == 1) {
        rc = run_op((size_t)g[0], ws, io, input_u8, s);
      } else if (kind == Route::ConvBurst) {
        const BurstParams* bp[kBurstGroupMax];
        for (size_t k = 0; k < g.size(); ++k) bp[k] = &std::get<BurstParams>(ws->route[g[k]].geom);
        rc = launch_conv_burst(bp, (int)g.size(), dtype, s);
      } else if (kind == Route::ConvT) {
        const ConvTParams* tp[kConvTGroupMax];
        for (size_t k = 0; k < g.size(); ++k) tp[k] = &std::get<ConvTParams>(ws->route[g[k]].geom);
        rc = launch_convt_group(tp, (int)g.size(), dtype, s);
      } else {  // Route::ConvLat
        const ConvParams* hp[kLatGroupMax];
        const ConvParams* dp[kLatGroupMax];
        for (size_t k = 0; k < g.size(); ++k) {
          hp[k] = &ws->params[g[k]];
          dp[k] = ws->dparams + g[k];
        }
        rc = launch_conv_lat_group(hp, dp, (int)g.size(), dtype, s, dtype == F32 && f32x3);
      }
      if (rc) return rc;
    }
    if (insitu) TV_HIP(hipEventRecord(ws->gev[gi], s));
    return TV_OK;
  }
  for (size_t k = op0; k < nops && k < op1; ++k) {  // positions op0 .. op1 - 1 of the execution order
    rc = run_op((size_t)ws->order[k], ws, io, input_u8, s);
    if (rc) return rc;
  }
  return TV_OK;
}

int Engine::prepare(int B, hipStream_t s) {
  TV_HIP(hipSetDevice(device));
  const std::vector<int> sz = slice_sizes(B);
  Workspace* ws = nullptr;
  if (sz.size() > 1) {
    SideStreams* ss = nullptr;
    int rc = get_side(s, (int)sz.size() - 1, &ss);
    if (rc) return rc;
    for (size_t k = 1; k < sz.size(); ++k) {
      rc = get_workspace(sz[k], ss->s[k - 1], &ws);
      if (rc) return rc;
    }
  }
  return get_workspace(sz[0], s, &ws);
}

// The caller's pointer arrays -> IoPtrs, refusing a count that is not the plan's
int Engine::check_io(const void* const* inputs, int n_in, float* const* outputs, int n_out, int B, IoPtrs* io) {
  if (B < 1) {
    set_error("batch must be >= 1");
    return TV_EINVAL;
  }
  if (n_in != (int)plan.ins.size() || n_out != (int)plan.outs.size()) {
    set_error("this model takes " + std::to_string(plan.ins.size()) + " input(s) and writes " +
              std::to_string(plan.outs.size()) + " output(s), got " + std::to_string(n_in) + " and " +
              std::to_string(n_out) + (n_in == 1 && n_out == 1 ? " (use tv_engine_forward_multi)" : ""));
    return TV_EINVAL;
  }
  bool ok = inputs && outputs;
  for (int i = 0; ok && i < n_in; ++i) ok = (io->in[i] = inputs[i]) != nullptr;
  for (int i = 0; ok && i < n_out; ++i) ok = (io->out[i] = outputs[i]) != nullptr;
  if (!ok) {
    set_error("null input/output pointer");
    return TV_EINVAL;
  }
  return TV_OK;
}

int Engine::forward(const void* input, int input_u8, int B, float* out, hipStream_t s) {
  return forward_multi(&input, 1, &out, 1, input_u8, B, s);
}

int Engine::forward_multi(const void* const* inputs, int n_in, float* const* outputs, int n_out, int input_u8, int B,
                          hipStream_t s) {
  IoPtrs io;
  int rc = check_io(inputs, n_in, outputs, n_out, B, &io);
  return rc ? rc : forward_io(io, input_u8, B, s);
}

int Engine::forward_io(const IoPtrs& io, int input_u8, int B, hipStream_t s) {
  TV_HIP(hipSetDevice(device));
  const std::vector<int> sz = slice_sizes(B);
  if (sz.size() > 1) {
    // frames are independent (no cross-frame state): slice 0 on `s`, the others on side
    // streams forked from and joined back into `s` (graph-capture safe: event fork / join)
    SideStreams* ss = nullptr;
    int rc = get_side(s, (int)sz.size() - 1, &ss);
    if (rc) return rc;
    // the buffers of the slice that starts at frame f0: every pointer advanced by its own frame size
    auto from = [&](size_t f0) {
      IoPtrs q;
      for (size_t i = 0; i < plan.ins.size(); ++i) {
        const IoSpec& t = plan.ins[i];
        const size_t in_frame = input_u8 ? (size_t)t.H * t.W * 3 : (size_t)t.C * t.H * t.W * 4;
        q.in[i] = (const char*)io.in[i] + f0 * in_frame;
      }
      for (size_t i = 0; i < plan.outs.size(); ++i) {
        const IoSpec& t = plan.outs[i];
        q.out[i] = io.out[i] + f0 * ((size_t)t.H * t.W * t.cpad);
      }
      return q;
    };
    // (diagnostic TV_SLICE_LAG = L: the other slices start once slice 0 has run its first L
    // ops, so that their heavy first layers meet slice 0's latency-bound deep levels — measured
    // slower: 4647 frames/s at L = 0, 4465 / 4338 / 4311 at L = 26 / 56 / 64, profiles/r4r)
    const size_t lag = std::min((size_t)slice_lag, plan.ops.size());
    if (lag) {
      rc = run_all(io, input_u8, sz[0], s, 0, lag);
      if (rc) return rc;
    }
    TV_HIP(hipEventRecord(ss->fork, s));
    size_t f0 = (size_t)sz[0];
    for (size_t k = 1; k < sz.size(); ++k) {
      TV_HIP(hipStreamWaitEvent(ss->s[k - 1], ss->fork, 0));
      rc = run_all(from(f0), input_u8, sz[k], ss->s[k - 1]);
      if (rc) return rc;
      f0 += (size_t)sz[k];
    }
    rc = run_all(io, input_u8, sz[0], s, lag, plan.ops.size());
    if (rc) return rc;
    for (size_t k = 1; k < sz.size(); ++k) {
      TV_HIP(hipEventRecord(ss->join[k - 1], ss->s[k - 1]));
      TV_HIP(hipStreamWaitEvent(s, ss->join[k - 1], 0));
    }
    return TV_OK;
  }
  return run_all(io, input_u8, B, s);
}

int Engine::forward_insitu(const void* input, int input_u8, int B, float* out, hipStream_t s, float* ms, int cap,
                           int* n_slices) {
  if (slice_lag) {
    set_error("forward_insitu: not with a slice lag");
    return TV_EINVAL;
  }
  profiled_u8 = input_u8;
  const int prev = insitu;
  insitu = 1;
  int rc = forward(input, input_u8, B, out, s);
  insitu = prev;
  if (rc) return rc;
  TV_HIP(hipStreamSynchronize(s));  // (the side slices are joined into s)
  return insitu_read(B, s, ms, cap, n_slices);
}

int Engine::insitu_read(int B, hipStream_t s, float* ms, int cap, int* n_slices) {
  int rc = 0;
  const std::vector<int> sz = slice_sizes(B);
  SideStreams* ss = nullptr;
  if (sz.size() > 1) {
    rc = get_side(s, (int)sz.size() - 1, &ss);
    if (rc) return rc;
  }
  const size_t nops = plan.ops.size();
  for (size_t k = 0; k < sz.size(); ++k) {
    Workspace* ws = nullptr;
    rc = get_workspace(sz[k], k ? ss->s[k - 1] : s, &ws);
    if (rc) return rc;
    if (ws->gev.size() != ws->groups.size() + 1) {
      set_error("forward_insitu: no events recorded");
      return TV_EINVAL;
    }
    for (size_t i = 0; i < nops && (int)i < cap; ++i) ms[k * cap + i] = 0.f;
    for (size_t gi = 0; gi < ws->groups.size(); ++gi) {
      float t = 0;
      TV_HIP(hipEventElapsedTime(&t, ws->gev[gi], ws->gev[gi + 1]));
      const int i = ws->groups[gi][0];
      if (i < cap) ms[k * cap + i] = t;
    }
  }
  *n_slices = (int)sz.size();
  return TV_OK;
}

const char* Engine::op_kernel(int B, size_t i) {
  std::lock_guard<std::mutex> g(mu);
  for (const auto& kv : workspaces) {
    if (kv.first.second != B) continue;
    Workspace* ws = kv.second;
    // the kernel instance as rocprofv3 demangles it (template <T, OutT, MODE or TW>)
    static const char* tn[3] = {"float", "_Float16", "__bf16"};
    const OpSpec& op = plan.ops[i];
    const OpRoute& r = ws->route[i];
    const std::string t = tn[dtype], o = op.out < 0 || op.out_f32 ? "float" : tn[dtype];
    const std::string mode = std::to_string(op.kind == OP_CONVT_ADD || op.up_s ? 1 : 0);
    const std::string smode = std::to_string(profiled_u8 ? (desc.in_w % 4 == 0 ? 2 : 1) : 0);  // input kind of the last profile()
    const char* x3 = dtype == F32 && f32x3 ? ", true>" : ">";
    auto str = [](int v) { return std::to_string(v); };
    std::string& name = ws->kname[i];
    switch (r.kind) {
      case Route::Staging: return "prep";
      case Route::StagingInStem: return "prep (fused into the stem)";
      case Route::StemInS2: return "(fused into block_layers.0.conv1: stem_s2)";
      case Route::StemS2: name = "tv::ss2::stem_s2<" + t + ", " + smode + ">"; break;
      case Route::Stem: name = "tv::stem::stem_conv<" + t + ", " + smode + ", " + (op.N <= 32 ? "1" : "4") + ">"; break;
      case Route::LayoutIn: name = "tv::nchw_to_nhwc<" + t + ">"; break;
      case Route::BilinearAdd: name = "tv::yh::bilinear_add<" + t + ">"; break;
      case Route::HeadScatter: name = "tv::yh::head_scatter"; break;
      case Route::MaxPool: name = "tv::dla::maxpool2_ceil<" + t + ">"; break;
      case Route::MaxPool3S2: name = "tv::rn::maxpool3x3s2<" + t + ">"; break;
      case Route::AddRelu: name = "tv::rn::add_relu<" + t + ">"; break;
      case Route::StoreF32: name = "tv::rn::store_f32<" + t + ">"; break;
      case Route::StemPool: name = "tv::rn::stem7s2_pool<" + t + ", " + (profiled_u8 ? "1>" : "0>"); break;
      case Route::StemInPool: name = "(fused into the max-pool: stem7s2_pool)"; break;
      case Route::DcnSample: name = "tv::dla::dcn_sample<" + t + ">"; break;
      case Route::DwConvTAdd: name = "tv::dla::dwconvt_add<" + t + ">"; break;
      case Route::ConvT: name = "tv::convt::convt_add<" + t + ", " + str(std::get<ConvTParams>(r.geom).np) + ">"; break;
      case Route::ConvT3: name = "tv::ct3::convt3<" + t + ", " + str(std::get<ConvT3Params>(r.geom).act) + ">"; break;
      case Route::ConvT3Done: name = "(fused into the phase (0,0) launch: convt3)"; break;
      case Route::HeadsDone: name = "(fused into the 3x3 heads)"; break;
      case Route::DcnInFused: name = "(sampled inside the fused DCNv2 kernel)"; break;
      case Route::DcnFused: {
        const DcnParams& d = std::get<DcnParams>(r.geom);
        const bool wide = d.N % 128 == 0;
        if ((dcn64_mode == 3 || dcn64_mode == 4) && dcn_win_supported(d)) {
          name = "tv::dcn::dcn_win<" + t + ">";
        } else if (dcn64_mode == 5 && d.C % 64 == 0 && d.om_ldc % 2 == 0) {
          name = "tv::dcn::dcn_gemm64d<" + t + (wide ? ", 128, 64>" : ", 64, 64>");
        } else if (dcn64_mode && d.C % 64 == 0) {  // dcn_gemm64<T, BN, PX>: the tile as launch_dcn_gemm picks it
          int bn, px;
          dcn64_tile(d, dcn64_mode, &bn, &px);
          name = "tv::dcn::dcn_gemm64<" + t + ", " + str(bn) + ", " + str(px) + ">";
          if (d.ksplit > 1) name += " split-K " + str(d.ksplit);
        } else {
          name = "tv::dcn::dcn_gemm<" + t + (wide ? ", 128>" : ", 64>");
        }
        break;
      }
      case Route::ConvSmall:
        name = std::string(csm_variant(op.segs[0].stride) ? "tv::csm::conv_small_halo<" : "tv::csm::conv_small<") + t + ", " +
               str(plan.tensors[op.segs[0].src].C) + ", " + str(op.N) + ", " + str(op.segs[0].stride) + ", " + str(op.act) + ">";
        break;
      case Route::ConvLat: name = "tv::lat::conv_lat<" + t + x3; break;
      case Route::ConvBurst: {
        const int q = (std::get<BurstParams>(r.geom).nk16 + 3) / 4;
        int kpw = 20;
        for (int v : {4, 6, 8, 12, 18, 20})
          if (q <= v) { kpw = v; break; }
        name = "tv::burst::conv_burst<" + t + ", " + str(kpw) + ">";
        break;
      }
      case Route::Conv1x1: name = "tv::c1x1::conv1x1_stream<" + t + (op.N > 64 ? ", 4>" : ", 2>"); break;
      case Route::Conv3x3S2: name = "tv::c3s2::conv3x3s2<" + t + ", " + str(op.act) + ">"; break;
      case Route::Conv3x3:
      case Route::HeadsFused: {
        const C3Geom& g = std::get<C3Geom>(r.geom);
        name = "tv::c3::conv3x3<" + t + ", " + t + ", " + str(g.tw) + ", " + str(op.act) + ", " +
               str(r.kind == Route::HeadsFused) + ", " + str(g.res) + ", " + str(g.ni) + ", " +
               str(plan.tensors[op.segs[0].src].C / 32) + ", " + str(g.nw) + ">";
        break;
      }
      case Route::ConvPipe:
        name = "tv::pipe::conv_pipe<" + t + ", " + o + ", " + mode + x3;
        if (ws->params[i].ksplit > 1) name += " split-K " + str(ws->params[i].ksplit);
        break;
      case Route::ConvIgemm: name = "tv::conv_igemm<" + t + ", " + o + ", " + mode + ">"; break;
    }
    return name.c_str();
  }
  return "";
}

int Engine::profile(const void* input, int input_u8, int B, float* out, hipStream_t s, float* ms, double* flops,
                    int cap, int* n_ops) {
  return profile_multi(&input, 1, &out, 1, input_u8, B, s, ms, flops, cap, n_ops);
}

int Engine::profile_multi(const void* const* inputs, int n_in, float* const* outputs, int n_out, int input_u8, int B,
                          hipStream_t s, float* ms, double* flops, int cap, int* n_ops) {
  IoPtrs io;
  int rc = check_io(inputs, n_in, outputs, n_out, B, &io);
  return rc ? rc : profile_io(io, input_u8, B, s, ms, flops, cap, n_ops);
}

int Engine::profile_io(const IoPtrs& io, int input_u8, int B, hipStream_t s, float* ms, double* flops, int cap,
                       int* n_ops) {
  profiled_u8 = input_u8;
  TV_HIP(hipSetDevice(device));
  Workspace* ws = nullptr;
  int rc = get_workspace(B, s, &ws);
  if (rc) return rc;
  const size_t n = plan.ops.size();
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) TV_HIP(hipEventCreate(&e));
  // one op per launch, in execution order (each op's time between its neighbours' events)
  TV_HIP(hipEventRecord(ev[0], s));
  for (size_t k = 0; k < n; ++k) {
    rc = run_op((size_t)ws->order[k], ws, io, input_u8, s);
    if (rc) {  // name the op (with AMD_SERIALIZE_KERNEL=3 a faulting launch reports here)
      set_error("op " + std::to_string(ws->order[k]) + " (" + plan.ops[ws->order[k]].label + "): " + tv_last_error());
      break;
    }
    TV_HIP(hipEventRecord(ev[k + 1], s));
  }
  if (!rc) {
    TV_HIP(hipEventSynchronize(ev[n]));
    for (size_t k = 0; k < n; ++k) {
      const int i = ws->order[k];
      if (i >= cap) continue;
      float t = 0;
      TV_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms[i] = t;
      flops[i] = plan.ops[i].flops * B;
    }
    // an op fused into another launch does its FLOPs there: the stem inside stem_s2 (block0.conv1's
    // launch), the block-diagonal 1x1 heads inside the 3x3 heads' epilogue. Their own rows launch
    // nothing (or only an in-place activation) and report no FLOPs.
    for (size_t i = 0; i < n && (int)i < cap; ++i) {
      int host = -1;
      const Route kind = ws->route[i].kind;
      if (kind == Route::StemInS2) host = ss2_op;
      else if (kind == Route::StemInPool) host = (int)i + 1;
      else if (kind == Route::HeadsDone) host = (int)i - 1;
      else if (kind == Route::ConvT3Done) host = (int)i - plan.ops[i].segs[0].convt_phase;
      if (host < 0 || host >= cap) continue;
      flops[host] += flops[i];
      flops[i] = 0.0;
    }
    *n_ops = (int)n;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

void Engine::op_stored(const Workspace* ws, size_t i, int32_t shape[4]) const {
  const OpSpec& op = plan.ops[i];
  shape[0] = shape[1] = shape[2] = shape[3] = 0;
  switch (ws->route[i].kind) {
    case Route::StagingInStem:  // never stored: the launch that does this op keeps its result on chip
    case Route::StemInS2:
    case Route::StemInPool:
    case Route::DcnInFused:
    case Route::HeadsFused:
    case Route::ConvT3Done:     // (the phase-(0,0) op reports the tensor the four phases share)
    case Route::HeadScatter:    // several of the caller's outputs, none of them an NHWC tensor
      return;
    default: break;
  }
  if (op.out < 0) {  // the caller's fp32 output buffer
    const IoSpec& o = plan.outspec(op.out);
    shape[0] = o.H, shape[1] = o.W, shape[2] = o.cpad, shape[3] = 4;
    return;
  }
  const TensorSpec& t = plan.tensors[op.out];
  shape[0] = t.H, shape[1] = t.W, shape[2] = t.C, shape[3] = t.f32 ? 4 : (int32_t)dtype_size(dtype);
}

int Engine::op_shapes(int B, hipStream_t s, int32_t (*shape)[4], int cap, int* n_ops) {
  TV_HIP(hipSetDevice(device));
  Workspace* ws = nullptr;
  int rc = get_workspace(B, s, &ws);
  if (rc) return rc;
  const size_t n = plan.ops.size();
  for (size_t i = 0; i < n && (int)i < cap; ++i) op_stored(ws, i, shape[i]);
  *n_ops = (int)n;
  return TV_OK;
}

int Engine::op_outputs(const void* input, int input_u8, int B, float* out, hipStream_t s, void* const* dst,
                       int n_dst) {
  return op_outputs_multi(&input, 1, &out, 1, input_u8, B, s, dst, n_dst);
}

int Engine::op_outputs_multi(const void* const* inputs, int n_in, float* const* outputs, int n_out, int input_u8, int B,
                             hipStream_t s, void* const* dst, int n_dst) {
  IoPtrs io;
  int rc = check_io(inputs, n_in, outputs, n_out, B, &io);
  if (rc) return rc;
  profiled_u8 = input_u8;
  TV_HIP(hipSetDevice(device));
  Workspace* ws = nullptr;
  rc = get_workspace(B, s, &ws);
  if (rc) return rc;
  for (size_t k = 0; k < plan.ops.size(); ++k) {
    const size_t i = (size_t)ws->order[k];
    rc = run_op(i, ws, io, input_u8, s);
    if (rc) {
      set_error("op " + std::to_string(i) + " (" + plan.ops[i].label + "): " + tv_last_error());
      return rc;
    }
    if ((int)i >= n_dst || !dst[i]) continue;
    int32_t sh[4];
    op_stored(ws, i, sh);
    const size_t bytes = (size_t)B * sh[0] * sh[1] * sh[2] * sh[3];
    const int o = plan.ops[i].out;  // (< 0: the op wrote the caller's output buffer, its data comes from there)
    const void* from = o < 0 ? (const void*)io.out[-1 - o] : (const char*)ws->arena + ws->off[o];
    if (bytes && from != dst[i]) TV_HIP(hipMemcpyAsync(dst[i], from, bytes, hipMemcpyDeviceToDevice, s));
  }
  return TV_OK;
}

}  // namespace tv
