"""stem7s2_pool (csrc/resnet.hip: conv1 7x7 / s2 + bn1 + ReLU + MaxPool2d(3, 2, 1) in one launch from
the fp32 NCHW image) against the unfused route (knob TV_RSTEM=0: the generic row-expanded stem GEMM,
then maxpool3x3s2), fp16 and bf16, on the pooled tensor both routes store (NativeEngine.op_outputs_multi).

Sizes. The kernel's tile is 4 x 6 pooled pixels (kTH x kTW). A 6 x 9 pooled map has one full and one
partial tile in both axes; it comes from conv maps of 11 or 12 rows and 17 or 18 columns, so both
parities of the conv size occur in both axes: images 21 x 33 (conv 11 x 17: the last pooled row and
column look at conv row 11 / column 17, outside the conv map), 24 x 36 (conv 12 x 18) and 21 x 36.

Bound. Both routes multiply the same operands — the image and the folded weights rounded to the
compute dtype, products exact in the fp32 accumulator — and differ only in the order of the
K + 1 = 148 fp32 additions (147 products and the shift) and so, at most, in the one rounding of the
result to the compute dtype. As tests/layer_ref.py derives it: each accumulator is within
148 * 2^-24 * A of the exact sum, A = sum |x_k| |w_k| + |shift|, so the two differ by at most twice
that, and their roundings by at most that plus one unit in the last place of the larger, 2 u |y|.
ReLU and the max over a window are 1-Lipschitz, so the pooled values differ by at most the largest
bound in their window. Nothing here is fitted to the kernels' output."""
import functools

import pytest
import torch
import torch.nn.functional as F

import resnet18_ref as rr

pytestmark = pytest.mark.gpu

U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
SIZES = [(21, 33), (24, 36), (21, 36)]
B = 2


@functools.lru_cache(maxsize=None)
def _weights(shift):
    sd = rr.seeded_resnet18_state_dict(seed=17)
    if shift:  # a large positive bn1 shift: a conv position computed from the zero padding alone is positive
        sd["bn1.bias"] = torch.full_like(sd["bn1.bias"], shift)
    return sd


def _pooled(sd, img, precision, knobs):
    from tauv_vision_amd import engine as tv_engine
    from tauv_vision_amd.yolact import Resnet101Backbone
    tv_engine.set_diagnostic_knobs(knobs)
    try:
        bb = Resnet101Backbone(None, precision=precision)
        bb.load_state_dict({"_feature_extractor." + k: v for k, v in sd.items()}, strict=True)
        taps = bb.forward_nhwc(img)
    finally:
        tv_engine.set_diagnostic_knobs(None)
    eng = next(iter(bb._engines.values()))
    rows = eng.op_outputs_multi([img], [torch.empty_like(t) for t in taps])
    (label, kernel, pooled), = [r for r in rows if r[0] == "maxpool"]
    stem, = [r for r in rows if r[0].startswith("conv1")]
    return kernel, pooled.float().cpu(), stem, [t.cpu() for t in taps]


@torch.no_grad()
def _bound(sd, img, precision):
    """Per pooled element, NHWC: the largest conv-position bound of its window (module docstring)."""
    dt, u = _DT[precision], U[precision]
    m = rr.resnet18_ref(sd)
    w, b = rr._fold(m.conv1, m.bn1)
    wq, xq = w.float().to(dt).double(), img.cpu().to(dt).double()
    A = F.conv2d(xq.abs(), wq.abs(), None, 2, 3) + b.abs()[None, :, None, None]
    y = F.conv2d(xq, wq, b, 2, 3)
    acc = 148 * 2.0 ** -24 * A
    d = 2 * acc + 2 * u * (y.abs() + acc)
    return F.max_pool2d(d, 3, 2, 1).permute(0, 2, 3, 1), F.max_pool2d(F.relu(y), 3, 2, 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("shift", [0.0, 5.0])
@pytest.mark.parametrize("H,W", SIZES)
def test_fused_stem_equals_unfused_route(H, W, shift, precision):
    sd = _weights(shift)
    img = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(H * W)).cuda()
    kf, fused, stem_f, taps_f = _pooled(sd, img, precision, None)
    ku, unfused, stem_u, taps_u = _pooled(sd, img, precision, {"TV_RSTEM": "0"})
    assert kf.startswith("tv::rn::stem7s2_pool<") and stem_f[2] is None, (kf, stem_f[1])
    assert ku.startswith("tv::rn::maxpool3x3s2<") and stem_u[2] is not None, (ku, stem_u[1])
    CH, CW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(stem_u[2].shape) == (B, CH, CW, 64)
    assert fused.shape == unfused.shape == (B, (CH - 1) // 2 + 1, (CW - 1) // 2 + 1, 64) == (B, 6, 9, 64)
    bound, ref = _bound(sd, img, precision)
    diff = (fused.double() - unfused.double()).abs()
    worst = float((diff / bound).max())
    print(f"stem {H}x{W} shift {shift} {precision}: max diff {float(diff.max()):.3e}, {worst:.3f} x bound, "
          f"{float((diff > 0).double().mean()):.3f} of the elements differ")
    assert (diff <= bound).all(), f"{worst} x the one-rounding bound"
    # both against the float64 pooled stem on the same rounded operands: one rounding of a value within the
    # accumulation error (no teeth lost to comparing two wrong routes with each other)
    for name, got in (("fused", fused), ("unfused", unfused)):
        assert ((got.double() - ref).abs() <= bound).all(), name
    if shift and (CH % 2 or CW % 2):
        # teeth: keeping the out-of-image conv positions (computed from the zero-padded image, relu(shift +
        # partial sum) > 0) in the max is outside the bound somewhere on these inputs
        m = rr.resnet18_ref(sd)
        with torch.no_grad():
            w, b = rr._fold(m.conv1, m.bn1)
        dt = _DT[precision]
        xq = F.pad(img.cpu().to(dt).double(), (3, 5, 3, 5))  # room for conv row CH / column CW
        y = F.relu(F.conv2d(xq, w.float().to(dt).double(), b, 2, 0))[:, :, :CH + 1, :CW + 1]
        y = F.pad(y, (1, 0, 1, 0))  # row / column -1 of the zero-padded image: relu(shift) > 0, but pad with 0 is enough
        wrong = F.max_pool2d(y, 3, 2, 0).permute(0, 2, 3, 1)[:, :6, :9]
        assert not ((wrong - ref).abs() <= bound).all(), "the kept-position error would pass unnoticed"
    for a in taps_f:
        assert torch.isfinite(a).all()
