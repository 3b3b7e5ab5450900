// Host-only weight packing (pack.h): BN folding and every weight layout the planners emit.
#include "pack.h"

#include <algorithm>
#include <cmath>
#include <set>

namespace tv {

void store_elem(void* base, size_t i, float v, int dtype) {
  if (dtype == F32) {
    reinterpret_cast<float*>(base)[i] = v;
  } else if (dtype == F16) {
    reinterpret_cast<_Float16*>(base)[i] = (_Float16)v;
  } else {
    reinterpret_cast<uint16_t*>(base)[i] = f32_to_bf16(v);
  }
}

std::vector<uint8_t> to_dtype(const std::vector<float>& m, int dtype) {
  std::vector<uint8_t> out(m.size() * dtype_size(dtype));
  for (size_t i = 0; i < m.size(); ++i) store_elem(out.data(), i, m[i], dtype);
  return out;
}

void place_weight(std::vector<float>& hw, int Kpad, int row0, size_t k0, const float* w, int n, int wcin, int taps,
                  int ci0, int cin, int cs, const double* scale, int re) {
  for (int co = 0; co < n; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int t = 0; t < taps; ++t) {
        const size_t k = re ? (size_t)(t / re) * cs + (t % re) * cin + ci : (size_t)t * cs + ci;
        const float v = w[((size_t)co * wcin + ci0 + ci) * taps + t];
        hw[(size_t)(row0 + co) * Kpad + k0 + k] = scale ? (float)((double)v * scale[co]) : v;
      }
}

namespace {

struct Packer {
  const Plan& plan;
  const HostWeights& host_w;
  int dtype, stem_op, ct3_mode;

  const float* weight(const std::string& name, int64_t numel) const;
  int fold(const std::string& conv, const std::string& bn, int cout, std::vector<double>& scale,
           std::vector<double>& shift) const;
  // the flavours: each fills its rows and columns of the op's staging matrix and bias
  struct Staging {
    std::vector<float> hw, bias;  // fp32 [Npad][Kpad], [Npad]
  };
  int dwconvt(const OpSpec& op, HostPacked& pk) const;
  int convt_add(const OpSpec& op, HostPacked& pk, Staging& st) const;
  int heads(const OpSpec& op, const HostPacked& pk, Staging& st) const;
  int identity_seg(const SegSpec& sg, int N, size_t k0, const HostPacked& pk, Staging& st) const;
  int convt_phase_seg(const OpSpec& op, const SegSpec& sg, int wN, int wcin, size_t k0, HostPacked& pk,
                      Staging& st) const;
  int conv_seg(const SegSpec& sg, int wN, int wcin, bool first, size_t k0, const HostPacked& pk, Staging& st) const;
  void head_fragments(const OpSpec& op, HostPacked& pk, const Staging& st) const;
  int pack_op(size_t oi, HostPacked& pk) const;
};

const float* Packer::weight(const std::string& name, int64_t numel) const {
  auto it = host_w.find(name);
  if (it == host_w.end()) {
    set_error("missing state_dict key: " + name);
    return nullptr;
  }
  if (it->second.second != numel) {
    set_error("state_dict key " + name + ": expected " + std::to_string(numel) + " elements, got " +
              std::to_string(it->second.second));
    return nullptr;
  }
  return it->second.first;
}

// Folded BN affine for a conv `p` (+ BatchNorm `bn`): scale, shift per output channel.
int Packer::fold(const std::string& conv, const std::string& bn, int cout, std::vector<double>& scale,
                 std::vector<double>& shift) const {
  scale.assign(cout, 1.0);
  shift.assign(cout, 0.0);
  // bias=False convs (DLA34, centerpoint_dla.py:24-27) have no `.bias` key in the layout
  std::vector<float> zeros;
  const float* b = nullptr;
  if (plan.names.count(conv + ".bias")) {
    b = weight(conv + ".bias", cout);
    if (!b) return TV_ENOTFOUND;
  } else {
    zeros.assign(cout, 0.f);
    b = zeros.data();
  }
  for (int i = 0; i < cout; ++i) shift[i] = b[i];
  if (bn.empty()) return TV_OK;
  const float* g = weight(bn + ".weight", cout);
  const float* be = weight(bn + ".bias", cout);
  const float* mu = weight(bn + ".running_mean", cout);
  const float* var = weight(bn + ".running_var", cout);
  if (!g || !be || !mu || !var) return TV_ENOTFOUND;
  for (int i = 0; i < cout; ++i) {
    double s = (double)g[i] / std::sqrt((double)var[i] + 1e-5);
    scale[i] = s;
    shift[i] = ((double)b[i] - (double)mu[i]) * s + (double)be[i];
  }
  return TV_OK;
}


// depthwise ConvTranspose2d (DLA-34's IDAUp) weight [C][1][2f][2f] -> fp32 [2f][2f][C]
int Packer::dwconvt(const OpSpec& op, HostPacked& pk) const {
  const int c = op.N, k = 2 * op.up_s;
  const float* w = weight(op.up_w + ".weight", (int64_t)c * k * k);
  if (!w) return TV_ENOTFOUND;
  std::vector<float> t((size_t)k * k * c);
  for (int co = 0; co < c; ++co)
    for (int tap = 0; tap < k * k; ++tap) t[(size_t)tap * c + co] = w[(size_t)co * k * k + tap];
  pk.w = to_dtype(t, F32);
  return TV_OK;
}

// ConvTranspose2d(k = s) + skip: weight [cin][c][s][s] -> row (i * s + j) * c + co per output phase (i, j)
int Packer::convt_add(const OpSpec& op, HostPacked& pk, Staging& st) const {
  const int c = op.N, s = op.up_s, cin = plan.tensors[op.src].C;
  const float* w = weight(op.up_w + ".weight", (int64_t)cin * c * s * s);
  const float* b = weight(op.up_w + ".bias", c);
  if (!w || !b) return TV_ENOTFOUND;
  for (int i = 0; i < s; ++i)
    for (int j = 0; j < s; ++j)
      for (int co = 0; co < c; ++co) {
        const int n = (i * s + j) * c + co;
        st.bias[n] = b[co];
        for (int ci = 0; ci < cin; ++ci) st.hw[(size_t)n * pk.Kpad + ci] = w[(((size_t)ci * c + co) * s + i) * s + j];
      }
  return TV_OK;
}

// stacked heads (3x3, single segment: head h's rows after head h - 1's) or block-diagonal 1x1 heads
// (head h's rows at diag_out_off[h], its input channels at diag_in_off[h])
int Packer::heads(const OpSpec& op, const HostPacked& pk, Staging& st) const {
  const SegSpec& sg = op.segs[0];
  const int cs = plan.tensors[sg.src].C;
  const bool diag = !op.diag_in_off.empty();
  int row = 0;
  for (size_t h = 0; h < op.stack_w.size(); ++h) {
    const int n = op.stack_n[h];
    const int cin = diag ? plan.tensors[sg.src].C / (int)op.stack_w.size() : sg.cin;
    const int k = sg.kh;
    const float* w = weight(op.stack_w[h] + ".weight", (int64_t)n * cin * k * k);
    const float* b = weight(op.stack_w[h] + ".bias", n);
    if (!w || !b) return TV_ENOTFOUND;
    const int r0 = diag ? op.diag_out_off[h] : row;
    const int c0 = diag ? op.diag_in_off[h] : 0;
    for (int co = 0; co < n; ++co) st.bias[r0 + co] = b[co];
    place_weight(st.hw, pk.Kpad, r0, c0, w, n, cin, k * k, 0, cin, cs);
    row += n;
  }
  return TV_OK;
}

// residual added as-is: identity 1x1 (exact in every compute dtype) ... or through an eval
// BatchNorm that follows a ReLU and so folds into no conv (YOLACT head blocks): the identity
// scaled per channel, the shift in the bias
int Packer::identity_seg(const SegSpec& sg, int N, size_t k0, const HostPacked& pk, Staging& st) const {
  std::vector<double> scale(N, 1.0), shift(N, 0.0);
  if (!sg.bn.empty()) {
    int rc = fold("", sg.bn, N, scale, shift);
    if (rc) return rc;
  }
  for (int co = 0; co < std::min(N, sg.cin); ++co) {
    st.hw[(size_t)co * pk.Kpad + k0 + co] = (float)scale[co];
    st.bias[co] += (float)shift[co];
  }
  return TV_OK;
}

// ConvTranspose2d(3, s2, p1) weight [cin][cout][3][3], one output parity (pi, pj): tap
// (dy, dx) of the phase conv reads input (m + dy, n + dx) and uses kernel element
// ky = 1 (pi = 0) or 2 - 2 dy (pi = 1) — out[2m + pi] += x[m + dy] W[ky] with
// 2m + pi = 2(m + dy) - 1 + ky — and kx likewise
int Packer::convt_phase_seg(const OpSpec& op, const SegSpec& sg, int wN, int wcin, size_t k0, HostPacked& pk,
                            Staging& st) const {
  const int cs = plan.tensors[sg.src].C;
  const float* w = weight(sg.wname + ".weight", (int64_t)wcin * wN * 9);
  if (!w) return TV_ENOTFOUND;
  std::vector<double> scale, shift;
  int rc = fold(sg.wname, "", wN, scale, shift);
  if (rc) return rc;
  for (int co = 0; co < wN; ++co) st.bias[co] += (float)shift[co];
  const int pi = sg.convt_phase >> 1, pj = sg.convt_phase & 1;
  for (int dy = 0; dy < sg.kh; ++dy)
    for (int dx = 0; dx < sg.kw; ++dx) {
      const int ky = pi == 0 ? 1 : 2 - 2 * dy, kx = pj == 0 ? 1 : 2 - 2 * dx;
      const int t = dy * sg.kw + dx;
      for (int co = 0; co < wN; ++co)
        for (int ci = 0; ci < sg.cin; ++ci)
          st.hw[(size_t)co * pk.Kpad + k0 + (size_t)t * cs + ci] =
              w[(((size_t)(sg.ci0 + ci) * wN + co) * 3 + ky) * 3 + kx];
    }
  // all four phases in one launch (convt3.hip): the phase-(0,0) op carries the whole
  // ConvTranspose2d's weight in that kernel's fragment order (knob TV_CT3=0: off)
  if (ct3_mode && dtype != F32 && sg.convt_phase == 0 && op.segs.size() == 1 && sg.ci0 == 0 &&
      sg.cin == cs && wcin == cs && convt3_supported(cs, wN, cs, wN, 1, 1, dtype_size(dtype))) {
    pk.w_ct3.resize(convt3_weight_bytes(cs, wN));
    convt3_pack(w, cs, wN, dtype, pk.w_ct3.data());
  }
  return TV_OK;
}

// a BN-folded conv segment, plain or over a row-expanded source; `first`: the first segment of
// its conv in this op, which adds the conv's folded shift to the bias
int Packer::conv_seg(const SegSpec& sg, int wN, int wcin, bool first, size_t k0, const HostPacked& pk,
                     Staging& st) const {
  const int re = sg.row_expand;  // row-expanded input: K index = ky * cs + kx * cin + c
  const int kk = re ? sg.kh * re : sg.kh * sg.kw;
  const float* w = weight(sg.wname + ".weight", (int64_t)wN * wcin * kk);
  if (!w) return TV_ENOTFOUND;
  std::vector<double> scale, shift;
  int rc = fold(sg.wname, sg.bn, wN, scale, shift);
  if (rc) return rc;
  if (first)
    for (int co = 0; co < wN; ++co) st.bias[co] += (float)shift[co];
  place_weight(st.hw, pk.Kpad, 0, k0, w, wN, wcin, kk, sg.ci0, sg.cin, plan.tensors[sg.src].C, scale.data(), re);
  return TV_OK;
}

// fused 1x1 heads (conv3x3 EPI 1): per 128-channel tile nt of the hidden (stacked 3x3) output,
// fragment (k-step j, lane l) = 8 weights W2[row0 + l%32][128nt + 16j + 8(l/32) + e]; reads the
// finished staging matrix and bias of the block-diagonal op
void Packer::head_fragments(const OpSpec& op, HostPacked& pk, const Staging& st) const {
  const int K = plan.tensors[op.segs[0].src].C;  // hidden channels
  const int nts = K / 128;
  const int hid = K / (int)op.stack_w.size();    // hidden channels per head
  bool ok = K % 128 == 0 && nts <= 16 && hid % 128 == 0;
  for (size_t h = 0; h < op.stack_n.size(); ++h) ok = ok && op.stack_n[h] <= 32;
  if (!ok) return;
  pk.head_w.assign((size_t)nts * 8 * 64 * 16, 0);
  pk.head_b.assign((size_t)nts * 32, 0.f);
  for (int nt = 0; nt < nts; ++nt) {
    const int h = nt * 128 / hid;
    const int row0 = op.diag_out_off[h], nr = op.stack_n[h];
    pk.head_row0[nt] = row0;
    pk.head_nrows[nt] = nr;
    if (nt * 128 == op.diag_in_off[h])
      for (int r = 0; r < nr; ++r) pk.head_b[nt * 32 + r] = st.bias[row0 + r];
    for (int j = 0; j < 8; ++j)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int r = l & 31, k = nt * 128 + 16 * j + 8 * (l >> 5) + e;
          const float v = r < nr ? st.hw[(size_t)(row0 + r) * pk.Kpad + k] : 0.f;
          store_elem(pk.head_w.data(), ((size_t)(nt * 8 + j) * 64 + l) * 8 + e, v, dtype);
        }
  }
}

int Packer::pack_op(size_t oi, HostPacked& pk) const {
  const OpSpec& op = plan.ops[oi];
  const int BK = 128 / dtype_size(dtype);
  if (op.kind == OP_DWCONVT_ADD) return dwconvt(op, pk);
  if (op.kind != OP_CONV && op.kind != OP_CONVT_ADD) return TV_OK;  // no weights
  // geometry: 128-byte k-steps per segment over its source's stored channels, rows padded to the tile
  const bool up = op.kind == OP_CONVT_ADD;
  pk.Npad = (int)align_up(up ? op.up_s * op.up_s * op.N : op.N, kTile);
  if (up) {
    pk.seg_ksteps = {(plan.tensors[op.src].C + BK - 1) / BK};
  } else {
    for (const SegSpec& sg : op.segs) pk.seg_ksteps.push_back((sg.kh * sg.kw * plan.tensors[sg.src].C + BK - 1) / BK);
  }
  int ksteps = 0;
  for (int ks : pk.seg_ksteps) ksteps += ks;
  pk.Kpad = ksteps * BK;
  Staging st{std::vector<float>((size_t)pk.Npad * pk.Kpad, 0.f), std::vector<float>(pk.Npad, 0.f)};
  int rc = TV_OK;
  if (up) {
    rc = convt_add(op, pk, st);
  } else if (!op.stack_w.empty()) {
    rc = heads(op, pk, st);
  } else {
    // segments in order; bias = sum over the distinct convs feeding this GEMM.
    // rows of the PyTorch weight: a plain conv into the caller's fp32 output stores out_cpad
    // columns of an out_c-channel conv (protonet _output_layer)
    const int wN = op.out < 0 ? plan.outspec(op.out).C : op.N;
    std::set<std::string> seen;
    int kb = 0;
    for (size_t si = 0; !rc && si < op.segs.size(); ++si) {
      const SegSpec& sg = op.segs[si];
      // total input channels of the PyTorch weight = max over segments sharing it
      int wcin = 0;
      for (const SegSpec& o : op.segs)
        if (o.wname == sg.wname) wcin = std::max(wcin, o.ci0 + o.cin);
      const size_t k0 = (size_t)kb * BK;
      rc = sg.identity           ? identity_seg(sg, op.N, k0, pk, st)
           : sg.convt_phase >= 0 ? convt_phase_seg(op, sg, wN, wcin, k0, pk, st)
                                 : conv_seg(sg, wN, wcin, seen.insert(sg.wname).second, k0, pk, st);
      kb += pk.seg_ksteps[si];
    }
  }
  if (rc) return rc;
  if (dtype != F32 && !op.diag_in_off.empty() && op.segs.size() == 1) head_fragments(op, pk, st);
  pk.w = to_dtype(st.hw, dtype);
  if ((int)oi == stem_op) {  // stem.hip streams its weights in MFMA B-fragment order
    std::vector<uint8_t> frag(stem_weight_bytes());
    stem_fragment_order(reinterpret_cast<const uint16_t*>(pk.w.data()), pk.Npad, pk.Kpad,
                        reinterpret_cast<uint16_t*>(frag.data()));
    pk.w.swap(frag);
  }
  pk.bias.swap(st.bias);
  return TV_OK;
}

}  // namespace

int pack_op_host(const Plan& plan, size_t oi, int dtype, const HostWeights& host_w, int stem_op, int ct3_mode,
                 HostPacked* out) {
  *out = HostPacked{};
  return Packer{plan, host_w, dtype, stem_op, ct3_mode}.pack_op(oi, *out);
}

}  // namespace tv
