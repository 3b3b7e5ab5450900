// Host-only weight packing: BatchNorm folding and the [Npad][Kpad] layouts the planners' ops are
// uploaded in. Nothing here calls the HIP runtime: Engine::pack_op uploads what pack_op_host
// returns, diag.cpp places the single-kernel tests' weights with the same primitive, and
// tv_diag_pack_op reports an op's bytes on a machine without a GPU.
#pragma once
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.h"
#include "planner.h"

namespace tv {

constexpr int kTile = 128;
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// state_dict key -> (fp32 data, element count): the caller's weight views, valid during create only
using HostWeights = std::unordered_map<std::string, std::pair<const float*, int64_t>>;

// One op's weights as they will be uploaded (every buffer empty for an op that has none)
struct HostPacked {
  int Npad = 0, Kpad = 0;
  std::vector<int> seg_ksteps;
  std::vector<uint8_t> w;     // [Npad][Kpad] compute dtype (the stem op: stem.hip's B-fragment order;
                              // OP_DWCONVT_ADD: fp32 [2f][2f][C])
  std::vector<float> bias;    // [Npad]
  std::vector<uint8_t> w_ct3; // convt3.hip fragments of a whole ConvTranspose2d(3, s2) (its phase-(0,0) op)
  // block-diagonal 1x1 heads whose fused epilogue is representable (conv3x3 EPI 1): MFMA A-fragments
  // and bias per 128-channel tile of the stacked 3x3 heads' output, and each tile's output rows
  std::vector<uint8_t> head_w;
  std::vector<float> head_b;
  int head_row0[16] = {}, head_nrows[16] = {};
};

void store_elem(void* base, size_t i, float v, int dtype);
std::vector<uint8_t> to_dtype(const std::vector<float>& m, int dtype);

// Input channels [ci0, ci0 + cin) of a PyTorch conv weight w [n][wcin][taps] into rows [row0, row0 + n)
// of the fp32 staging matrix hw (row length Kpad) from column k0 on: tap-major, channel-minor over
// the source's `cs` stored channels, so tap t's channel ci lands at k0 + t * cs + ci; re > 0 (a
// row-expanded source holding `re` horizontal taps per pixel) at k0 + (t / re) * cs + (t % re) * cin + ci.
// scale != null: each row times scale[co], the product formed in double.
void place_weight(std::vector<float>& hw, int Kpad, int row0, size_t k0, const float* w, int n, int wcin, int taps,
                  int ci0, int cin, int cs, const double* scale = nullptr, int re = 0);

// Op `oi` of the plan in compute dtype `dtype`; stem_op / ct3_mode as Engine::configure left them.
// TV_ENOTFOUND (tv_last_error set) for a missing state_dict key or a wrong element count.
int pack_op_host(const Plan& plan, size_t oi, int dtype, const HostWeights& host_w, int stem_op, int ct3_mode,
                 HostPacked* out);

}  // namespace tv
