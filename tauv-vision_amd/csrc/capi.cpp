// extern "C" boundary (include/tauv_vision_amd.h). No exceptions cross it.
#include <cstring>
#include <new>
#include <string>

#include "engine.h"

namespace tv {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tv

using namespace tv;

#define TV_GUARD(...)                                      \
  try {                                                    \
    __VA_ARGS__                                            \
  } catch (const std::bad_alloc&) {                        \
    set_error("host allocation failed");                   \
    return TV_ENOMEM;                                      \
  } catch (const std::exception& e) {                      \
    set_error(e.what());                                   \
    return TV_EINVAL;                                      \
  } catch (...) {                                          \
    set_error("unknown C++ exception");                    \
    return TV_EINVAL;                                      \
  }

struct tv_engine {
  Engine e;
};

extern "C" {

const char* tv_last_error(void) { return g_err.c_str(); }
const char* tv_version(void) { return "tauv-vision_amd 0.1 (gfx950)"; }

int tv_model_param_count(const tv_model_desc* d, int32_t* count) {
  TV_GUARD({
    if (!d || !count) { set_error("null argument"); return TV_EINVAL; }
    Plan p;
    int rc = build_plan(*d, &p);
    if (rc) return rc;
    *count = (int32_t)p.params.size();
    return TV_OK;
  })
}

int tv_model_param_info(const tv_model_desc* d, int32_t i, char* name, int32_t cap, int64_t shape[4], int32_t* ndim) {
  TV_GUARD({
    if (!d || !name || !shape || !ndim) { set_error("null argument"); return TV_EINVAL; }
    Plan p;
    int rc = build_plan(*d, &p);
    if (rc) return rc;
    if (i < 0 || i >= (int)p.params.size()) { set_error("param index out of range"); return TV_EINVAL; }
    const ParamInfo& pi = p.params[i];
    if ((int)pi.name.size() + 1 > cap) { set_error("name buffer too small"); return TV_EINVAL; }
    std::memcpy(name, pi.name.c_str(), pi.name.size() + 1);
    *ndim = (int32_t)pi.shape.size();
    for (size_t k = 0; k < 4; ++k) shape[k] = k < pi.shape.size() ? pi.shape[k] : 0;
    return TV_OK;
  })
}

int tv_model_geometry(const tv_model_desc* d, double* flops, int32_t* oh, int32_t* ow, int32_t* oc, int32_t* ocp) {
  TV_GUARD({
    if (!d) { set_error("null argument"); return TV_EINVAL; }
    Plan p;
    int rc = build_plan(*d, &p);
    if (rc) return rc;
    if (flops) *flops = p.flops_per_frame;
    if (oh) *oh = p.out_h;
    if (ow) *ow = p.out_w;
    if (oc) *oc = p.out_c;
    if (ocp) *ocp = p.out_cpad;
    return TV_OK;
  })
}

int tv_model_io(const tv_model_desc* d, int32_t* n_in, int32_t in_shape[TV_MAX_IO][3], int32_t* n_out,
                int32_t out_shape[TV_MAX_IO][4]) {
  TV_GUARD({
    if (!d || !n_in || !in_shape || !n_out || !out_shape) { set_error("null argument"); return TV_EINVAL; }
    Plan p;
    int rc = build_plan(*d, &p);
    if (rc) return rc;
    *n_in = (int32_t)p.ins.size();
    *n_out = (int32_t)p.outs.size();
    for (size_t i = 0; i < p.ins.size() && i < TV_MAX_IO; ++i)
      in_shape[i][0] = p.ins[i].C, in_shape[i][1] = p.ins[i].H, in_shape[i][2] = p.ins[i].W;
    for (size_t i = 0; i < p.outs.size() && i < TV_MAX_IO; ++i)
      out_shape[i][0] = p.outs[i].H, out_shape[i][1] = p.outs[i].W, out_shape[i][2] = p.outs[i].C,
      out_shape[i][3] = p.outs[i].cpad;
    return TV_OK;
  })
}

int tv_engine_forward_multi(tv_engine* e, const float* const* inputs, int32_t n_in, float* const* outputs,
                            int32_t n_out, int32_t B, void* stream) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    return e->e.forward_multi(reinterpret_cast<const void* const*>(inputs), n_in, outputs, n_out, 0, B,
                              (hipStream_t)stream);
  })
}

// u8 camera frames feed only a plan whose one input is the image (staged by its first op); the archs
// that take feature maps (OP_LAYOUT_IN) refuse them before anything is launched
static int takes_frames(const Plan& p) {
  bool ok = p.ins.size() == 1;
  for (const OpSpec& op : p.ops) ok = ok && op.kind != OP_LAYOUT_IN;
  if (!ok) set_error("this model takes an fp32 NCHW feature map, not u8 frames");
  return ok ? TV_OK : TV_EINVAL;
}

int tv_engine_forward_multi_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* const* outputs, int32_t n_out,
                               void* stream) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    int rc = takes_frames(e->e.plan);
    if (rc) return rc;
    const void* in = frames;
    return e->e.forward_multi(&in, 1, outputs, n_out, 1, B, (hipStream_t)stream);
  })
}

int tv_engine_op_outputs_multi_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* const* outputs, int32_t n_out,
                                  void* stream, void* const* dst, int32_t n_dst) {
  TV_GUARD({
    if (!e || (n_dst > 0 && !dst) || n_dst < 0) { set_error("bad argument"); return TV_EINVAL; }
    int rc = takes_frames(e->e.plan);
    if (rc) return rc;
    const void* in = frames;
    return e->e.op_outputs_multi(&in, 1, outputs, n_out, 1, B, (hipStream_t)stream, dst, n_dst);
  })
}

int tv_engine_profile_multi_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* const* outputs, int32_t n_out,
                               void* stream, float* ms, double* flops, int32_t cap, int32_t* n_ops) {
  TV_GUARD({
    if (!e || !ms || !flops || !n_ops) { set_error("null argument"); return TV_EINVAL; }
    int rc = takes_frames(e->e.plan);
    if (rc) return rc;
    const void* in = frames;
    int n = 0;
    rc = e->e.profile_multi(&in, 1, outputs, n_out, 1, B, (hipStream_t)stream, ms, flops, cap, &n);
    *n_ops = n;
    return rc;
  })
}

int tv_engine_profile_multi(tv_engine* e, const float* const* inputs, int32_t n_in, float* const* outputs,
                            int32_t n_out, int32_t B, void* stream, float* ms, double* flops, int32_t cap,
                            int32_t* n_ops) {
  TV_GUARD({
    if (!e || !ms || !flops || !n_ops) { set_error("null argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.profile_multi(reinterpret_cast<const void* const*>(inputs), n_in, outputs, n_out, 0, B,
                                (hipStream_t)stream, ms, flops, cap, &n);
    *n_ops = n;
    return rc;
  })
}

int tv_diag_bilinear_add(const void* src, int32_t B, int32_t src_h, int32_t src_w, int32_t src_ldc, void* dst,
                         int32_t dst_h, int32_t dst_w, int32_t dst_ldc, int32_t C, int32_t dtype, void* stream) {
  TV_GUARD({
    return launch_bilinear_add(src, B, src_h, src_w, src_ldc, dst, dst_h, dst_w, dst_ldc, C, dtype,
                               (hipStream_t)stream);
  })
}

int tv_engine_create(const tv_model_desc* d, const tv_weight_view* w, int32_t n, int32_t device, tv_engine** out) {
  TV_GUARD({
    if (!d || !out || (n && !w)) { set_error("null argument"); return TV_EINVAL; }
    tv_engine* e = new tv_engine();
    int rc = e->e.create(*d, w, n, device);
    if (rc) {
      delete e;
      return rc;
    }
    *out = e;
    return TV_OK;
  })
}

// "NAME=VALUE;NAME=VALUE" -> pairs (tv_engine_create_diag, tv_diag_pack_op)
static int parse_knobs(const char* knobs, std::vector<std::pair<std::string, std::string>>* kv) {
  for (const char* c = knobs ? knobs : ""; *c;) {
    const char* e = c;
    while (*e && *e != ';') ++e;
    std::string item(c, e);
    c = *e ? e + 1 : e;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) { set_error("engine knob without '=': " + item); return TV_EINVAL; }
    kv->emplace_back(item.substr(0, eq), item.substr(eq + 1));
  }
  return TV_OK;
}

int tv_engine_create_diag(const tv_model_desc* d, const tv_weight_view* w, int32_t n, int32_t device,
                          const char* knobs, tv_engine** out) {
  TV_GUARD({
    if (!d || !out || (n && !w)) { set_error("null argument"); return TV_EINVAL; }
    std::vector<std::pair<std::string, std::string>> kv;
    int rc = parse_knobs(knobs, &kv);
    if (rc) return rc;
    tv_engine* e = new tv_engine();
    rc = e->e.create(*d, w, n, device, kv);
    if (rc) {
      delete e;
      return rc;
    }
    *out = e;
    return TV_OK;
  })
}

int tv_diag_pack_op(const tv_model_desc* d, const tv_weight_view* w, int32_t n, const char* knobs, int32_t op,
                    int32_t info[5], char* label, int32_t label_cap, int32_t (*segs)[6], int32_t seg_cap,
                    int64_t size[3], void* weight, void* bias, void* extra, const int64_t cap[3]) {
  TV_GUARD({
    if (!d || !info || !size || (n && !w) || seg_cap < 0 || (seg_cap && !segs) || ((weight || bias || extra) && !cap)) {
      set_error("null argument");
      return TV_EINVAL;
    }
    std::vector<std::pair<std::string, std::string>> kv;
    int rc = parse_knobs(knobs, &kv);
    if (rc) return rc;
    Engine e;
    HostWeights host_w;
    if ((rc = weight_views(w, n, &host_w)) || (rc = e.configure(*d, kv, 256))) return rc;
    info[0] = (int32_t)e.plan.ops.size();
    if (op < 0 || op >= info[0]) { set_error("op index out of range"); return TV_EINVAL; }
    const OpSpec& o = e.plan.ops[op];
    HostPacked hp;
    if ((rc = pack_op_host(e.plan, op, e.dtype, host_w, e.stem_op, e.ct3_mode, &hp))) return rc;
    info[1] = o.kind; info[2] = hp.Npad; info[3] = hp.Kpad; info[4] = (int32_t)o.segs.size();
    if (label && label_cap > 0) {
      std::strncpy(label, o.label.c_str(), label_cap - 1);
      label[label_cap - 1] = 0;
    }
    for (int i = 0; i < info[4] && i < seg_cap; ++i) {
      const SegSpec& sg = o.segs[i];
      const int32_t row[6] = {sg.kh, sg.row_expand ? sg.row_expand : sg.kw, e.plan.tensors[sg.src].C, sg.ci0, sg.cin,
                              i < (int)hp.seg_ksteps.size() ? hp.seg_ksteps[i] : 0};
      std::memcpy(segs[i], row, sizeof(row));
    }
    // extra: the convt3 fragments, or the fused-head fragments + their fp32 bias + head_row0 / head_nrows
    std::vector<uint8_t> ex = hp.w_ct3;
    if (!hp.head_w.empty()) {
      ex = hp.head_w;
      const uint8_t* b = reinterpret_cast<const uint8_t*>(hp.head_b.data());
      ex.insert(ex.end(), b, b + hp.head_b.size() * sizeof(float));
      for (const int* a : {hp.head_row0, hp.head_nrows})
        ex.insert(ex.end(), reinterpret_cast<const uint8_t*>(a), reinterpret_cast<const uint8_t*>(a + 16));
    }
    size[0] = (int64_t)hp.w.size(); size[1] = (int64_t)(hp.bias.size() * sizeof(float)); size[2] = (int64_t)ex.size();
    if (weight && size[0] && cap[0] == size[0]) std::memcpy(weight, hp.w.data(), size[0]);
    if (bias && size[1] && cap[1] == size[1]) std::memcpy(bias, hp.bias.data(), size[1]);
    if (extra && size[2] && cap[2] == size[2]) std::memcpy(extra, ex.data(), size[2]);
    return TV_OK;
  })
}

int tv_engine_destroy(tv_engine* e) {
  TV_GUARD({
    delete e;
    return TV_OK;
  })
}

int tv_engine_prepare(tv_engine* e, int32_t B, void* stream) {
  TV_GUARD({
    if (!e || B < 1) { set_error("bad argument"); return TV_EINVAL; }
    return e->e.prepare(B, (hipStream_t)stream);
  })
}

int tv_engine_trim(tv_engine* e) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    return e->e.trim();
  })
}

int tv_engine_forward(tv_engine* e, const float* img, int32_t B, float* out, void* stream) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    return e->e.forward(img, 0, B, out, (hipStream_t)stream);
  })
}

int tv_engine_forward_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* out, void* stream) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    return e->e.forward(frames, 1, B, out, (hipStream_t)stream);
  })
}

int tv_engine_profile(tv_engine* e, const float* img, int32_t B, float* out, void* stream, float* ms, double* flops,
                      int32_t cap, int32_t* n_ops) {
  TV_GUARD({
    if (!e || !ms || !flops || !n_ops) { set_error("null argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.profile(img, 0, B, out, (hipStream_t)stream, ms, flops, cap, &n);
    *n_ops = n;
    return rc;
  })
}

int tv_engine_profile_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* out, void* stream, float* ms,
                         double* flops, int32_t cap, int32_t* n_ops) {
  TV_GUARD({
    if (!e || !ms || !flops || !n_ops) { set_error("null argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.profile(frames, 1, B, out, (hipStream_t)stream, ms, flops, cap, &n);
    *n_ops = n;
    return rc;
  })
}

int tv_engine_set_insitu(tv_engine* e, int32_t on) {
  TV_GUARD({
    if (!e) { set_error("null engine"); return TV_EINVAL; }
    e->e.insitu = on ? 1 : 0;
    return TV_OK;
  })
}

int tv_engine_insitu_read(tv_engine* e, int32_t B, void* stream, float* ms, int32_t cap, int32_t* n_slices) {
  TV_GUARD({
    if (!e || !ms || !n_slices || cap < 1 || B < 1) { set_error("bad argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.insitu_read(B, (hipStream_t)stream, ms, cap, &n);
    *n_slices = n;
    return rc;
  })
}

int tv_engine_forward_insitu(tv_engine* e, const float* img, int32_t B, float* out, void* stream, float* ms,
                             int32_t cap, int32_t* n_slices) {
  TV_GUARD({
    if (!e || !img || !out || !ms || !n_slices || cap < 1) { set_error("null argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.forward_insitu(img, 0, B, out, (hipStream_t)stream, ms, cap, &n);
    *n_slices = n;
    return rc;
  })
}

int tv_engine_forward_insitu_u8(tv_engine* e, const uint8_t* frames, int32_t B, float* out, void* stream, float* ms,
                                int32_t cap, int32_t* n_slices) {
  TV_GUARD({
    if (!e || !frames || !out || !ms || !n_slices || cap < 1) { set_error("null argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.forward_insitu(frames, 1, B, out, (hipStream_t)stream, ms, cap, &n);
    *n_slices = n;
    return rc;
  })
}

const char* tv_engine_op_label(tv_engine* e, int32_t i) {
  if (!e || i < 0 || i >= (int)e->e.plan.ops.size()) return "";
  return e->e.plan.ops[i].label.c_str();
}

int tv_engine_slices(tv_engine* e, int32_t B, int32_t* n, int32_t sb[TV_MAX_SLICES]) {
  TV_GUARD({
    if (!e || !n || !sb || B < 1) { set_error("bad argument"); return TV_EINVAL; }
    const std::vector<int> sz = e->e.slice_sizes(B);
    *n = (int32_t)sz.size();
    for (int k = 0; k < TV_MAX_SLICES; ++k) sb[k] = k < (int)sz.size() ? sz[k] : 0;
    return TV_OK;
  })
}

const char* tv_engine_op_kernel(tv_engine* e, int32_t B, int32_t i) {
  if (!e || i < 0 || i >= (int)e->e.plan.ops.size()) return "";
  return e->e.op_kernel(B, i);
}

int tv_engine_op_shapes(tv_engine* e, int32_t B, void* stream, int32_t (*shape)[4], int32_t cap, int32_t* n_ops) {
  TV_GUARD({
    if (!e || !shape || !n_ops || cap < 0 || B < 1) { set_error("bad argument"); return TV_EINVAL; }
    int n = 0;
    int rc = e->e.op_shapes(B, (hipStream_t)stream, shape, cap, &n);
    *n_ops = n;
    return rc;
  })
}

int tv_engine_op_outputs(tv_engine* e, const void* input, int32_t input_u8, int32_t B, float* out, void* stream,
                         void* const* dst, int32_t n_dst) {
  TV_GUARD({
    if (!e || (n_dst > 0 && !dst) || n_dst < 0) { set_error("bad argument"); return TV_EINVAL; }
    return e->e.op_outputs(input, input_u8 ? 1 : 0, B, out, (hipStream_t)stream, dst, n_dst);
  })
}

int tv_engine_op_outputs_multi(tv_engine* e, const float* const* inputs, int32_t n_in, float* const* outputs,
                               int32_t n_out, int32_t B, void* stream, void* const* dst, int32_t n_dst) {
  TV_GUARD({
    if (!e || (n_dst > 0 && !dst) || n_dst < 0) { set_error("bad argument"); return TV_EINVAL; }
    return e->e.op_outputs_multi(reinterpret_cast<const void* const*>(inputs), n_in, outputs, n_out, 0, B,
                                 (hipStream_t)stream, dst, n_dst);
  })
}

int tv_preprocess_u8(const uint8_t* frames, int32_t B, int32_t src_h, int32_t src_w, int32_t dst_h, int32_t dst_w,
                     float* img_nchw, void* stream) {
  TV_GUARD({
    if (!frames || !img_nchw) { set_error("null argument"); return TV_EINVAL; }
    return launch_preprocess_u8(frames, B, src_h, src_w, dst_h, dst_w, img_nchw, (hipStream_t)stream);
  })
}

int tv_heatmap_nms(const float* heat, const int64_t st[4], int32_t B, int32_t C, int32_t H, int32_t W, int32_t k,
                   int32_t apply_sigmoid, float* out, void* stream) {
  TV_GUARD({
    if (k < 1 || k % 2 == 0) { set_error("kernel_size must be odd and >= 1"); return TV_EINVAL; }
    if (!heat || !st || !out || B < 0 || C < 0 || H < 0 || W < 0) { set_error("bad argument"); return TV_EINVAL; }
    return launch_peaks(heat, st, B, C, H, W, k, apply_sigmoid, out, (hipStream_t)stream);
  })
}

int tv_heatmap_topk(const float* peaks, int32_t B, int64_t n, int32_t K, float* score, int32_t* index, void* stream) {
  TV_GUARD({
    if (!peaks || !score || !index || B < 1) { set_error("bad argument"); return TV_EINVAL; }
    return launch_topk(peaks, B, n, K, score, index, (hipStream_t)stream);
  })
}

int tv_index_split(const int32_t* flat, int32_t B, int32_t K, int32_t H, int32_t W, int64_t* index, int64_t* label,
                   void* stream) {
  TV_GUARD({
    if (!flat || !index || !label || B < 0 || K < 0 || H < 1 || W < 1) { set_error("bad argument"); return TV_EINVAL; }
    return launch_index_split(flat, B, K, H, W, index, label, (hipStream_t)stream);
  })
}

int tv_yolact_box_decode(const float* enc, const float* anchor, int32_t B, int32_t A, int32_t anchor_batch, float v0,
                         float v1, float* box, void* stream) {
  TV_GUARD({
    if (!enc || !anchor || !box) { set_error("bad argument"); return TV_EINVAL; }
    return launch_yolact_box_decode(enc, anchor, B, A, anchor_batch, v0, v1, box, (hipStream_t)stream);
  })
}

int tv_yolact_box_encode(const float* box, const float* anchor, int32_t B, int32_t A, int32_t anchor_batch, float v0,
                         float v1, float* enc, void* stream) {
  TV_GUARD({
    if (!enc || !anchor || !box) { set_error("bad argument"); return TV_EINVAL; }
    return launch_yolact_box_encode(box, anchor, B, A, anchor_batch, v0, v1, enc, (hipStream_t)stream);
  })
}

int tv_yolact_nms_workspace_size(int32_t B, int32_t A, int32_t top_k, int64_t* bytes) {
  TV_GUARD({
    if (!bytes || B < 1 || A < 1 || top_k < 1) { set_error("bad argument"); return TV_EINVAL; }
    const size_t n = yolact_nms_workspace_bytes(B, A, top_k);
    if (!n) return TV_EHIP;
    *bytes = (int64_t)n;
    return TV_OK;
  })
}

int tv_yolact_fast_nms_batched(const float* cls, int32_t B, int32_t A, int32_t C1, const float* box, int32_t top_k,
                               float iou_thr, float conf_thr, int64_t* det, int32_t* n_det, void* ws, int64_t ws_bytes,
                               void* stream) {
  TV_GUARD({
    if (!cls || !box || !det || !n_det || !ws || ws_bytes < 0) { set_error("bad argument"); return TV_EINVAL; }
    const int K = top_k < A ? top_k : A;
    return launch_yolact_fast_nms(cls, (long long)A * C1, A, C1, box, (long long)A * 4, B, top_k, iou_thr, conf_thr,
                                  ws, (size_t)ws_bytes, (long long*)det, K, n_det, (hipStream_t)stream);
  })
}

int tv_yolact_fast_nms(const float* cls, int32_t A, int32_t C1, const float* box, int32_t top_k, float iou_thr,
                       float conf_thr, int64_t* det, int32_t* n_det, void* stream) {
  TV_GUARD({
    if (!cls || !box || !det || !n_det || A < 1 || top_k < 1) { set_error("bad argument"); return TV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const size_t need = yolact_nms_workspace_bytes(1, A, top_k);
    if (!need) return TV_EHIP;
    void* ws = nullptr;
    TV_HIP(hipMallocAsync(&ws, need, s));
    const int K = top_k < A ? top_k : A;
    int rc = launch_yolact_fast_nms(cls, (long long)A * C1, A, C1, box, (long long)A * 4, 1, top_k, iou_thr, conf_thr,
                                    ws, need, (long long*)det, K, n_det, s);
    TV_HIP(hipFreeAsync(ws, s));
    return rc;
  })
}

int tv_yolact_assemble_mask(const float* proto, const int64_t pst[3], int32_t K, int32_t H, int32_t W,
                            const float* coeff, const float* box, int32_t n, float* mask, void* stream) {
  TV_GUARD({
    if (n == 0) return TV_OK;
    if (!proto || !pst || !coeff || !mask || n < 0) { set_error("bad argument"); return TV_EINVAL; }
    const long long st[4] = {0, pst[0], pst[1], pst[2]};
    return launch_yolact_assemble_mask(proto, st, 1, K, H, W, coeff, box, nullptr, nullptr, 0, n, mask,
                                       (hipStream_t)stream);
  })
}

int tv_yolact_assemble_masks(const float* proto, const int64_t pst[4], int32_t B, int32_t K, int32_t H, int32_t W,
                             const float* coeff, const float* box, const int32_t* counts, int32_t n_max, float* mask,
                             void* stream) {
  TV_GUARD({
    if (n_max == 0) return TV_OK;
    if (!proto || !pst || !coeff || !mask || n_max < 0) { set_error("bad argument"); return TV_EINVAL; }
    const long long st[4] = {pst[0], pst[1], pst[2], pst[3]};
    return launch_yolact_assemble_mask(proto, st, B, K, H, W, coeff, box, counts, nullptr, 0, n_max, mask,
                                       (hipStream_t)stream);
  })
}

int tv_yolact_assemble_masks_indexed(const float* proto, const int64_t pst[4], int32_t B, int32_t K, int32_t H,
                                     int32_t W, const float* coeff, const float* box, int32_t A, const int64_t* det,
                                     const int32_t* counts, int32_t n_max, float* mask, void* stream) {
  TV_GUARD({
    if (n_max == 0) return TV_OK;
    if (!proto || !pst || !coeff || !det || !counts || !mask || n_max < 0 || A < 1) {
      set_error("bad argument");
      return TV_EINVAL;
    }
    const long long st[4] = {pst[0], pst[1], pst[2], pst[3]};
    return launch_yolact_assemble_mask(proto, st, B, K, H, W, coeff, box, counts, (const long long*)det, A, n_max,
                                       mask, (hipStream_t)stream);
  })
}

int tv_yolact_detection_records(const float* cls, const float* box, const int64_t* det, const int32_t* counts, int32_t B,
                                int32_t A, int32_t C1, int32_t n_max, float* records, float* confidence, void* stream) {
  TV_GUARD({ return launch_yolact_detection_records(cls, box, (const long long*)det, counts, B, A, C1, n_max, records,
                                                    confidence, (hipStream_t)stream); })
}

int tv_localize_boxes(const float* records, int32_t rec_stride, const int32_t* counts, int32_t B, int32_t K,
                      const uint16_t* depth, int32_t depth_batch, int32_t dh, int32_t dw, double box_scale, double fx,
                      double fy, double cx, double cy, double min_depth_sum, double min_z, float* out, void* stream) {
  TV_GUARD({ return launch_localize_boxes(records, rec_stride, counts, B, K, depth, depth_batch, dh, dw, box_scale, fx,
                                          fy, cx, cy, min_depth_sum, min_z, out, (hipStream_t)stream); })
}

int tv_localize_masks(const float* masks, int32_t mh, int32_t mw, const int32_t* counts, const int64_t* det,
                      const float* box, int32_t A, int32_t B, int32_t n, const uint16_t* depth, int32_t depth_batch,
                      int32_t dh, int32_t dw, int32_t bound_by_box, double fx, double fy, double cx, double cy,
                      double min_depth_sum, double min_z, float* out, void* stream) {
  TV_GUARD({ return launch_localize_masks(masks, mh, mw, counts, (const long long*)det, box, A, B, n, depth,
                                          depth_batch, dh, dw, bound_by_box, fx, fy, cx, cy, min_depth_sum, min_z, out,
                                          (hipStream_t)stream); })
}

int tv_yolact_frame_masks(const float* masks, int32_t mh, int32_t mw, const int32_t* counts, int32_t B, int32_t n,
                          int32_t H, int32_t W, int32_t mode, int32_t bound_by_box, const int64_t* det, const float* box,
                          int32_t A, const uint8_t* frames, const float* records, const uint8_t* palette,
                          int32_t n_colours, uint32_t* bits, int32_t* area, uint8_t* overlay, void* stream) {
  TV_GUARD({ return launch_yolact_frame_masks(masks, mh, mw, counts, B, n, H, W, mode, bound_by_box,
                                              (const long long*)det, box, A, frames, records, palette, n_colours, bits,
                                              area, overlay, (hipStream_t)stream); })
}

int tv_match_keypoints(const float* obj_records, const int32_t* obj_counts, const float* kp_records,
                       const int32_t* kp_counts, const int32_t* owner_label, const int32_t* owner_slot,
                       int32_t n_keypoints, int32_t max_slots, int32_t B, int32_t K, int32_t K_kp, int32_t* kp_det,
                       int32_t* slot_kp, int32_t* n_matched, void* stream) {
  TV_GUARD({ return launch_match_keypoints(obj_records, obj_counts, kp_records, kp_counts, owner_label, owner_slot,
                                           n_keypoints, max_slots, B, K, K_kp, kp_det, slot_kp, n_matched,
                                           (hipStream_t)stream); })
}

int tv_solve_poses(const float* obj_records, const int32_t* obj_counts, const float* kp_records,
                   const int32_t* kp_counts, const int32_t* slot_kp, const float* model_points, int32_t n_labels,
                   int32_t max_slots, int32_t B, int32_t K, int32_t K_kp, int32_t in_h, int32_t in_w, float fx, float fy,
                   float cx, float cy, int32_t min_points, float* poses, void* stream) {
  TV_GUARD({ return launch_solve_poses(obj_records, obj_counts, kp_records, kp_counts, slot_kp, model_points, n_labels,
                                       max_slots, B, K, K_kp, in_h, in_w, fx, fy, cx, cy, min_points, poses,
                                       (hipStream_t)stream); })
}

int tv_evaluate_detections(const float* records, int32_t rec_stride, const int32_t* counts, const int32_t cols[6],
                           int32_t B, int32_t K, const uint8_t* truth_valid, const int64_t* truth_label,
                           const float* truth_center, const float* truth_size, int32_t N, int32_t mode,
                           double match_threshold, const float* score_thresholds, int32_t T, int32_t* det_truth,
                           int64_t* totals, void* stream) {
  TV_GUARD({ return launch_evaluate_detections(records, rec_stride, counts, cols, B, K, truth_valid,
                                               (const long long*)truth_label, truth_center, truth_size, N, mode,
                                               match_threshold, score_thresholds, T, det_truth, (long long*)totals,
                                               (hipStream_t)stream); })
}

int tv_yolact_mask_overlap(const uint32_t* bits, const int32_t* counts, const uint8_t* seg, const uint8_t* truth_valid,
                           int32_t B, int32_t K, int32_t N, int32_t H, int32_t W, int32_t* inter, int32_t* det_area,
                           int32_t* truth_area, void* stream) {
  TV_GUARD({ return launch_yolact_mask_overlap(bits, counts, seg, truth_valid, B, K, N, H, W, inter, det_area,
                                               truth_area, (hipStream_t)stream); })
}

int tv_yolact_evaluate_match(const float* confidence, const float* records, const int32_t* counts,
                             const uint8_t* truth_valid, const int64_t* truth_label, const float* truth_box,
                             const int32_t* inter, const int32_t* det_area, const int32_t* truth_area,
                             const float* iou_thresholds, int32_t B, int32_t K, int32_t N, int32_t C, int32_t T,
                             int64_t* cursor, int32_t* log, int64_t capacity, int32_t* det_truth, int64_t* totals,
                             void* stream) {
  TV_GUARD({ return launch_yolact_evaluate_match(confidence, records, counts, truth_valid,
                                                 (const long long*)truth_label, truth_box, inter, det_area, truth_area,
                                                 iou_thresholds, B, K, N, C, T, (long long*)cursor, log,
                                                 (long long)capacity, det_truth, (long long*)totals,
                                                 (hipStream_t)stream); })
}

int tv_augment_workspace_size(int32_t B, int32_t src_h, int32_t src_w, int64_t* bytes) {
  TV_GUARD({
    long long b = 0;
    const int rc = augment_workspace_size(B, src_h, src_w, bytes ? &b : nullptr);
    if (rc == 0) *bytes = (int64_t)b;
    return rc;
  })
}

int tv_augment_frames(const uint8_t* frames, const uint8_t* seg, int32_t B, int32_t src_h, int32_t src_w,
                      int32_t dst_h, int32_t dst_w, const float* records, uint64_t seed, const float mean[3],
                      const float std[3], float* img_out, uint8_t* seg_out, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  TV_GUARD({ return launch_augment_frames(frames, seg, B, src_h, src_w, dst_h, dst_w, records,
                                          (unsigned long long)seed, mean, std, img_out, seg_out, workspace,
                                          (long long)workspace_bytes, (hipStream_t)stream); })
}

int tv_decode_workspace_size(int32_t B, int32_t C, int32_t H, int32_t W, int32_t K, int64_t* bytes) {
  if (!bytes || B < 1 || C < 1 || H < 1 || W < 1 || K < 1) { set_error("bad argument"); return TV_EINVAL; }
  *bytes = (int64_t)decode_workspace_bytes(B, C, H, W, K);
  return TV_OK;
}

int tv_decode(const float* heat, const int64_t hs[4], const float* size, const int64_t ss[4], const float* offset,
              const int64_t os[4], const float* depth, const int64_t ds[4], int32_t B, int32_t C, int32_t H, int32_t W,
              int32_t K, int32_t mode, int32_t ratio, int32_t in_h, int32_t in_w, float thr, const float* aux,
              const int64_t aux_st[5], float* records, int32_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  TV_GUARD({
    int64_t need = 0;
    int rc = tv_decode_workspace_size(B, C, H, W, K, &need);
    if (rc) return rc;
    if (!heat || !hs || !size || !ss || !records || !counts || !ws || ws_bytes < need) {
      set_error("bad argument or workspace too small");
      return TV_EINVAL;
    }
    if (mode == 0 && (!offset || !os)) { set_error("decode needs the offset head"); return TV_EINVAL; }
    if (depth && !ds) { set_error("depth strides missing"); return TV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    DecodeParams p{};
    p.B = B; p.K = K; p.C = C; p.H = H; p.W = W;
    p.size = size;
    p.offset = offset;
    p.depth = depth;
    for (int i = 0; i < 4; ++i) {
      p.size_st[i] = ss[i];
      p.offset_st[i] = offset ? os[i] : 0;
      p.depth_st[i] = depth ? ds[i] : 0;
    }
    p.depth_mode = mode == 0 ? 0 : 1;
    p.pos_mode = mode == 0 ? 0 : 1;
    p.ratio = ratio; p.in_h = in_h; p.in_w = in_w;
    p.out_h = ratio > 0 ? in_h / ratio : H;
    p.out_w = ratio > 0 ? in_w / ratio : W;
    p.score_thr = thr;
    p.aux = aux;
    if (aux) {
      if (!aux_st) { set_error("aux strides missing"); return TV_EINVAL; }
      for (int i = 0; i < 5; ++i) p.aux_st[i] = aux_st[i];
    }
    p.records = records;
    p.counts = counts;
    return launch_decode(heat, hs, B, C, H, W, K, ws, (size_t)ws_bytes, p, s);
  })
}

int tv_decode_angles(const float* records, int32_t rec_stride, const int32_t* counts, const float* roll_bin,
                     const int64_t roll_bin_strides[4], const float* roll_offset, const int64_t roll_offset_strides[4],
                     const float* pitch_bin, const int64_t pitch_bin_strides[4], const float* pitch_offset,
                     const int64_t pitch_offset_strides[4], const float* yaw_bin, const int64_t yaw_bin_strides[4],
                     const float* yaw_offset, const int64_t yaw_offset_strides[4], const float* theta_range, int32_t B,
                     int32_t C, int32_t H, int32_t W, int32_t K, float* angles, void* stream) {
  TV_GUARD({
    AngleParams p{};
    p.records = records; p.rec_stride = rec_stride; p.counts = counts;
    const float* bins[3] = {roll_bin, pitch_bin, yaw_bin};
    const float* offs[3] = {roll_offset, pitch_offset, yaw_offset};
    const int64_t* bst[3] = {roll_bin_strides, pitch_bin_strides, yaw_bin_strides};
    const int64_t* ost[3] = {roll_offset_strides, pitch_offset_strides, yaw_offset_strides};
    for (int a = 0; a < 3; ++a) {
      p.bin[a] = bins[a];
      p.off[a] = offs[a];
      if ((bins[a] && !bst[a]) || (offs[a] && !ost[a])) { set_error("decode_angles: head strides missing"); return TV_EINVAL; }
      for (int i = 0; i < 4; ++i) {
        p.bin_st[a][i] = bins[a] ? bst[a][i] : 0;
        p.off_st[a][i] = offs[a] ? ost[a][i] : 0;
      }
    }
    p.theta_range = theta_range;
    p.B = B; p.C = C; p.H = H; p.W = W; p.K = K;
    p.angles = angles;
    return launch_decode_angles(p, (hipStream_t)stream);
  })
}

int tv_diag_dcn_conv(const void* x, const void* om, int32_t B, int32_t H, int32_t W, int32_t C, int32_t om_ldc,
                     const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, int32_t variant,
                     void* out, void* stream) {
  TV_GUARD({ return tv::diag_dcn_conv(x, om, B, H, W, C, om_ldc, weight, bias, N, act, dtype, variant, out,
                                      (hipStream_t)stream); })
}

int tv_diag_conv1x1(const void* const* src, const int32_t* C, const int32_t* ldc, int32_t nseg, int32_t M,
                    const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, void* out,
                    int32_t out_ldc, void* stream) {
  TV_GUARD({ return tv::diag_conv1x1(src, C, ldc, nseg, M, weight, bias, N, act, dtype, out, out_ldc,
                                     (hipStream_t)stream); })
}

int tv_diag_conv_burst(const void* const* src, const int32_t* geom, int32_t nseg, int32_t B, int32_t Ho, int32_t Wo,
                       const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, void* out,
                       int32_t out_ldc, void* stream) {
  TV_GUARD({ return tv::diag_conv_burst(src, geom, nseg, B, Ho, Wo, weight, bias, N, act, dtype, out, out_ldc,
                                        (hipStream_t)stream); })
}

int tv_diag_burst_plan(const int32_t* geom, int32_t nseg, int32_t B, int32_t Ho, int32_t Wo, int32_t N, int32_t* out) {
  TV_GUARD({ return tv::diag_burst_plan(geom, nseg, B, Ho, Wo, N, out); })
}

int tv_diag_conv_small(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldc, const float* weight,
                       const float* bias, int32_t N, int32_t stride, int32_t act, int32_t dtype, int32_t variant,
                       void* out, int32_t out_ldc, void* stream) {
  TV_GUARD({ return tv::diag_conv_small(src, B, H, W, C, ldc, weight, bias, N, stride, act, dtype, variant, out,
                                        out_ldc, (hipStream_t)stream); })
}

int tv_diag_convt3(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldc, const float* weight,
                   const float* bias, int32_t N, int32_t act, int32_t dtype, int32_t tile_w, int32_t tile_h, void* out,
                   int32_t out_ldc, void* stream) {
  TV_GUARD({ return tv::diag_convt3(src, B, H, W, C, ldc, weight, bias, N, act, dtype, tile_w, tile_h, out, out_ldc,
                                    (hipStream_t)stream); })
}

int tv_diag_convt_add(const void* src, int32_t B, int32_t h, int32_t w, int32_t src_ldc, const float* weight,
                      const float* bias, int32_t s, const void* add, int32_t add_ldc, void* out, int32_t out_ldc,
                      int32_t tH, int32_t tW, int32_t sy, int32_t sx, int32_t dtype, int32_t cus, int32_t* np,
                      void* stream) {
  TV_GUARD({ return tv::diag_convt_add(src, B, h, w, src_ldc, weight, bias, s, add, add_ldc, out, out_ldc, tH, tW, sy,
                                       sx, dtype, cus, np, (hipStream_t)stream); })
}

int tv_train_heatmap(const uint8_t* valid, const int64_t* label, const float* center, int32_t B, int32_t n_objects,
                     int32_t n_labels, int32_t in_h, int32_t in_w, int32_t downsample_ratio, double sigma,
                     float* heatmap, void* stream) {
  TV_GUARD({
    return tv::launch_train_heatmap(valid, reinterpret_cast<const long long*>(label), center, B, n_objects, n_labels,
                                    in_h, in_w, downsample_ratio, sigma, heatmap, (hipStream_t)stream);
  })
}

int tv_train_keypoint_targets(const uint8_t* keypoint_valid, const int64_t* keypoint_label,
                              const float* keypoint_center, const int64_t* keypoint_object_index, const float* center,
                              int32_t B, int32_t n_instances, int32_t n_objects, int32_t n_keypoints, int32_t in_h,
                              int32_t in_w, int32_t downsample_ratio, double heatmap_sigma, double affinity_sigma,
                              float* heatmap, float* affinity_weight, float* affinity, void* stream) {
  TV_GUARD({
    return tv::launch_train_keypoints(keypoint_valid, reinterpret_cast<const long long*>(keypoint_label),
                                      keypoint_center, reinterpret_cast<const long long*>(keypoint_object_index),
                                      center, B, n_instances, n_objects, n_keypoints, in_h, in_w, downsample_ratio,
                                      heatmap_sigma, affinity_sigma, heatmap, affinity_weight, affinity,
                                      (hipStream_t)stream);
  })
}

int tv_centernet_loss_workspace_size(const tv_loss_desc* desc, int64_t* bytes) {
  TV_GUARD({
    long long n = 0;
    const int rc = tv::centernet_loss_workspace_size(desc, bytes ? &n : nullptr);
    if (rc == TV_OK) *bytes = n;
    return rc;
  })
}

int tv_centernet_loss_dense(const tv_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({ return tv::launch_centernet_loss_dense(desc, workspace, workspace_bytes, (hipStream_t)stream); })
}

int tv_centernet_loss_objects(const tv_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({ return tv::launch_centernet_loss_objects(desc, workspace, workspace_bytes, (hipStream_t)stream); })
}

int tv_centernet_loss_finalize(const tv_loss_desc* desc, const void* workspace, int64_t workspace_bytes, float* out,
                               void* stream) {
  TV_GUARD({
    return tv::launch_centernet_loss_finalize(desc, workspace, workspace_bytes, out, (hipStream_t)stream);
  })
}

int tv_centernet_loss_scale(void* grad, int32_t dtype, int64_t n, const float* scale, void* stream) {
  TV_GUARD({ return tv::launch_centernet_loss_scale(grad, dtype, n, scale, (hipStream_t)stream); })
}

int tv_yolact_loss_workspace_size(const tv_yolact_loss_desc* desc, int64_t* bytes) {
  TV_GUARD({
    long long n = 0;
    const int rc = tv::yolact_loss_workspace_size(desc, bytes ? &n : nullptr);
    if (rc == TV_OK) *bytes = n;
    return rc;
  })
}

int tv_yolact_loss_match(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_MATCH, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_select(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_SELECT, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_anchors(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_ANCHORS, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_mask_sums(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_MASK_SUMS, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_mask(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_MASK, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_mask_coeff(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_MASK_COEFF, desc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
  })
}

int tv_yolact_loss_finalize(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, float* out,
                            void* stream) {
  TV_GUARD({
    return tv::launch_yolact_loss(tv::TV_YOLACT_LOSS_FINALIZE, desc, workspace, workspace_bytes, out, (hipStream_t)stream);
  })
}

}  // extern "C"
