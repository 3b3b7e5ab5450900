"""CenterpointDLA34's bandwidth kernels on their own (csrc/dla34.hip through tv_diag_dwconvt_add and
tv_diag_maxpool2), at the instances and geometries the DLA-34 plan never asks for.

launch_dwconvt_add picks dwconvt_add_p2<T, 1|2|3> (f = 2, 4, 8 on a power-of-two count of 16-byte
channel chunks) or the generic dwconvt_add<T>. The plan only has f = 2 and 4, 64 / 128 / 256 channels and
shifts of 0 or 1: the f = 8 instance and the whole generic kernel ran in no test before this file.

dwconvt_add against float64 F.conv_transpose2d(groups=C, stride=f, padding=f // 2) +
oracle.ref_dla34.pad_to_match + skip, from the tensors as stored (the fp32 depthwise weight is read as
it is: no operand is rounded). The kernel sums in fp64 (dla34.hip `acc[e] += (double)t.v[e] * (double)wp[e]`,
then `acc[e] + (double)s.v[e]`). Per output element, with A = sum |x| |w| + |skip| over its at most 2 x 2 taps:
  * every product is exact in fp64 (at most 24 + 24 bits); the at most four adds and the add of the skip value
    are each within 2^-53 of a partial sum <= A, and the float64 reference sums the same terms with the same
    error:  e64 = 10 2^-53 A between the two;
  * the sum is rounded to fp32 (2^-24) and then to T (store_vec `(T)o.v[i]`: u, plus ETA = half the smallest
    subnormal, yolact_layer_ref.ETA; none for fp32 tensors);
  det = e64 + (2^-24 + u (1 + 2^-24)) (|ref| + e64) + ETA     (u = 2^-11 fp16, 2^-8 bf16, 0 for fp32 tensors).
sy and sx are the planner's (planner_dla34.cpp ida(): max(0, (hu - tH) / 2), likewise W), which is what
pad_to_match does to a map larger than its target: the cases choose the target size that gives each
(sy, sx) in {0, 1, 3}^2, alternating the parity of the excess so that both "shifted" (excess 2 s) and
"shifted, then cropped" (2 s + 1) occur on each axis, plus the equal, crop-only and larger targets.

The generic and the _p2 kernel "take the same taps in the same order: identical results" (dla34.hip):
the launcher cannot be steered to the generic kernel at a power-of-two chunk count, so the first 48
channels of a 64-channel problem are run as a problem of their own (6 or 12 chunks: generic) and compared
bit for bit with the 64-channel run (_p2).

maxpool2_ceil against F.max_pool2d(x, 2, 2, ceil_mode=True), bit for bit: H, W in {1, 2, 7, 8} (a
window that is all over-hang but one pixel, odd sizes whose last window hangs over, even sizes),
normal and all-negative inputs (the -inf start value must never survive; a window that read its
neighbour in the next row or frame would return that larger value).

Measured on MI355X (largest |err| / det over the 13 target sizes of each row; recorded under
"dla34_aux/..." in profiles/layers/dla34_layers_gpu.json): 0.995-0.999 in fp16, bf16 and fp32 on every kernel,
the generic one at f = 3 and f = 4 included (one rounding of the fp64 sum: ~1.0 by construction). The generic
and _p2 kernels agree bit for bit at f = 2, 4, 8 in the three dtypes; maxpool2_ceil is bit-equal on all 16
sizes; the refusals write nothing.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import record_measurement
from oracle.ref_dla34 import pad_to_match

pytestmark = pytest.mark.gpu

_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
U_OUT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp32": 0.0}
ETA = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134, "fp32": 0.0}
SRC_H, SRC_W, BATCH = 5, 7, 2
TAIL = 256  # guard elements behind the output


def up_size(n, f):
    return (n - 1) * f - 2 * (f // 2) + 2 * f


def make_case(C, f, tH, tW, add_ldc, precision, seed):
    """(src, weight [C, 1, 2f, 2f], skip [B, tH, tW, add_ldc]) as stored, on the CPU."""
    dt = _DT[precision]
    g = torch.Generator().manual_seed(seed)
    src = torch.randn((BATCH, SRC_H, SRC_W, C), generator=g).to(dt)
    w = torch.randn((C, 1, 2 * f, 2 * f), generator=g) * 0.5
    skip = torch.randn((BATCH, tH, tW, add_ldc), generator=g).to(dt)
    return src, w, skip


def reference(src, w, skip, f, tH, tW):
    """(float64 NHWC reference, A) from the stored tensors."""
    C = src.shape[3]
    x = src.double().permute(0, 3, 1, 2)
    s = skip[..., :C].double().permute(0, 3, 1, 2)
    kw = dict(stride=f, padding=f // 2, groups=C)
    shape = torch.Size((x.shape[0], C, tH, tW))
    ref = pad_to_match(F.conv_transpose2d(x, w.double(), None, **kw), shape) + s
    A = pad_to_match(F.conv_transpose2d(x.abs(), w.double().abs(), None, **kw), shape) + s.abs()
    return ref.permute(0, 2, 3, 1).contiguous(), A.permute(0, 2, 3, 1).contiguous()


def run_kernel(src, w, skip, f, tH, tW, sy, sx, precision, expect_ok=True):
    """out [B, tH, tW, C] on the CPU (None if the launcher refused; then nothing was written)."""
    from tauv_vision_amd import _lib
    B, h, wd, C = src.shape
    dt = _DT[precision]
    n = B * tH * tW * C
    out = torch.full((n + TAIL,), float("nan"), dtype=dt).cuda()
    sd, kd = src.cuda(), skip.cuda()
    wdev = w[:, 0].permute(1, 2, 0).contiguous().float().cuda()  # [2f][2f][C], tap-major
    rc = _lib.lib().tv_diag_dwconvt_add(ctypes.c_void_p(sd.data_ptr()), B, h, wd, C, ctypes.c_void_p(wdev.data_ptr()), f,
                                        ctypes.c_void_p(kd.data_ptr()), skip.shape[3], ctypes.c_void_p(out.data_ptr()),
                                        tH, tW, sy, sx, _lib.DTYPES[precision], _lib.stream_of(sd.device))
    torch.cuda.synchronize()
    got = out.cpu()
    if not expect_ok:
        assert rc == _lib.TV_EINVAL, rc
        assert _lib.lib().tv_last_error()
        assert torch.isnan(got.float()).all(), "a refused launch wrote something"
        return None
    _lib.check(rc, "dwconvt_add")
    assert torch.isnan(got[n:].float()).all(), "wrote past the output"
    return got[:n].reshape(B, tH, tW, C)


def judge(got, ref, A, precision):
    """max |err| / det."""
    u = U_OUT[precision]
    e64 = 10 * 2.0 ** -53 * A
    det = e64 + (2.0 ** -24 + u * (1 + 2.0 ** -24)) * (ref.abs() + e64) + ETA[precision]
    err = (got.double() - ref).abs()
    assert not torch.isnan(got.float()).any()
    r = torch.where(err == 0, torch.zeros_like(err), err / det.clamp_min(1e-300))
    return float(r.max())


def target(f, sy, sx):
    """The target size whose pad_to_match shift is (sy, sx): excess 2 s or 2 s + 1, the parity alternating."""
    hu, wu = up_size(SRC_H, f), up_size(SRC_W, f)
    tH, tW = hu - 2 * sy - (sy + sx) % 2, wu - 2 * sx - (sy + sx + 1) % 2
    assert max(0, (hu - tH) // 2) == sy and max(0, (wu - tW) // 2) == sx and tH >= 1 and tW >= 1
    return tH, tW


SHIFTS = [(sy, sx) for sy in (0, 1, 3) for sx in (0, 1, 3)]
# (C, f, dtypes): the three _p2 instances; the generic kernel through f = 3 and through 6 chunks
KERNELS = [(64, 2, ("fp16", "bf16", "fp32")), (64, 4, ("fp16", "bf16", "fp32")), (64, 8, ("fp16", "bf16", "fp32")),
           (48, 3, ("fp16",)), (48, 4, ("fp16",))]


@pytest.mark.parametrize("C,f,precision", [(C, f, p) for C, f, ps in KERNELS for p in ps])
def test_dwconvt_add_matches_float64(C, f, precision):
    hu, wu = up_size(SRC_H, f), up_size(SRC_W, f)
    # every shift, then: equal; crop only (by 1); crop by 2f - 1 (shift f - 1, then crop); a larger target
    sizes = [target(f, sy, sx) for sy, sx in SHIFTS]
    sizes += [(hu, wu), (hu - 1, wu - 1), (hu - (2 * f - 1), wu - (2 * f - 1)), (hu + 2, wu + 1)]
    worst = 0.0
    for i, (tH, tW) in enumerate(sizes):
        if tH < 1 or tW < 1:
            continue
        sy, sx = max(0, (hu - tH) // 2), max(0, (wu - tW) // 2)
        add_ldc = C + (16 if i % 2 else 0)  # every other case reads the skip through a wider tensor
        src, w, skip = make_case(C, f, tH, tW, add_ldc, precision, 1000 * f + 10 * i + C)
        ref, A = reference(src, w, skip, f, tH, tW)
        got = run_kernel(src, w, skip, f, tH, tW, sy, sx, precision)
        r = judge(got, ref, A, precision)
        print(f"C={C} f={f} {precision} target {tH}x{tW} (up {hu}x{wu}) sy={sy} sx={sx} ldc={add_ldc}: {r:.3f} x det")
        assert r <= 1.0, (tH, tW, sy, sx, add_ldc, r)
        worst = max(worst, r)
    record_measurement(f"dla34_aux/dwconvt_add/C{C}/f{f}/{precision}", {"det_ratio": worst, "cases": len(sizes)})


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("f", [2, 4, 8])
def test_dwconvt_generic_and_p2_agree_bit_for_bit(f, precision):
    """The first 48 channels as a problem of their own (6 / 12 chunks: dwconvt_add<T>) against the
    64-channel run (4 / 8 / 16 chunks: dwconvt_add_p2<T, log2 f>), shifted and cropped both ways."""
    for sy, sx in ((1, 3), (3, 0), (0, 0)):
        tH, tW = target(f, sy, sx)
        src, w, skip = make_case(64, f, tH, tW, 80, precision, 77 + f)
        p2 = run_kernel(src, w, skip, f, tH, tW, sy, sx, precision)
        gen = run_kernel(src[..., :48].contiguous(), w[:48].contiguous(), skip, f, tH, tW, sy, sx, precision)
        assert torch.equal(gen, p2[..., :48]), (f, precision, sy, sx)


def test_dwconvt_add_refusals_write_nothing():
    f, (tH, tW) = 2, target(2, 1, 1)
    for C, precision in ((12, "fp16"), (6, "fp32"), (60, "bf16")):  # not whole 16-byte chunks
        src, w, skip = make_case(C, f, tH, tW, 64, precision, 5)
        assert run_kernel(src, w, skip, f, tH, tW, 1, 1, precision, expect_ok=False) is None
    src, w, skip = make_case(64, f, tH, tW, 64, "fp16", 6)
    assert run_kernel(src, w, skip, f, tH, tW, -1, 1, "fp16", expect_ok=False) is None
    assert run_kernel(src, w, skip, f, tH, tW, 1, -1, "fp16", expect_ok=False) is None
    assert run_kernel(src, w, skip, f, tH, tW, 1, 1, "fp16") is not None  # (the same call, valid)


def _maxpool(x, precision, expect_ok=True, C=None):
    from tauv_vision_amd import _lib
    B, H, W, Cx = x.shape
    C = C or Cx
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    n = B * Ho * Wo * Cx
    out = torch.full((n + TAIL,), float("nan"), dtype=x.dtype).cuda()
    xd = x.cuda()
    rc = _lib.lib().tv_diag_maxpool2(ctypes.c_void_p(xd.data_ptr()), B, H, W, C, ctypes.c_void_p(out.data_ptr()),
                                     _lib.DTYPES[precision], _lib.stream_of(xd.device))
    torch.cuda.synchronize()
    got = out.cpu()
    if not expect_ok:
        assert rc == _lib.TV_EINVAL, rc
        assert torch.isnan(got.float()).all(), "a refused launch wrote something"
        return None
    _lib.check(rc, "maxpool2")
    assert torch.isnan(got[n:].float()).all(), "wrote past the output"
    return got[:n].reshape(B, Ho, Wo, Cx)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("C", [16, 512])
def test_maxpool2_ceil_is_bit_equal_to_torch(C, precision):
    dt, B = _DT[precision], 3
    for H in (1, 2, 7, 8):
        for W in (1, 2, 7, 8):
            g = torch.Generator().manual_seed(100 * H + W + C)
            for negative in (False, True):
                x = torch.randn((B, H, W, C), generator=g)
                if negative:  # (a zero or -inf left by a window that found no pixel would show)
                    x = -(x.abs() + 0.25)
                x = x.to(dt)
                ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2, ceil_mode=True)
                ref = ref.permute(0, 2, 3, 1).contiguous().to(dt)
                got = _maxpool(x, precision)
                assert got.shape == ref.shape == (B, (H + 1) // 2, (W + 1) // 2, C)
                assert torch.equal(got, ref), (H, W, C, negative)
                assert not torch.isinf(got.float()).any()
                if negative:
                    assert float(got.float().max()) < 0


def test_maxpool2_refuses_partial_chunks():
    for C, precision in ((12, "fp16"), (6, "fp32"), (4, "bf16")):
        x = torch.zeros((1, 4, 4, 16), dtype=_DT[precision])
        assert _maxpool(x, precision, expect_ok=False, C=C) is None
