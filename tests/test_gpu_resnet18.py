"""The native ResNet-18 backbone and the whole-model plan on the GPU (TV_ARCH_RESNET18 / TV_ARCH_YOLACT:
csrc/planner_resnet.cpp, csrc/resnet.hip) against the float64 restatement of the reference backbone
(tests/resnet18_ref.py — torchvision is not available here, so parity with it is not pinned) and
tests/yolact_head_ref.py.

Bars: maxpool3x3s2 and add_relu bit-equal to torch; the fp32 / fp32x3 taps within 1e-4 * max(1, |ref|max),
the project's fp32 bar; the fp16 / bf16 taps within 3x the error of the restatement's own low-precision
emulation against float64 on the same inputs and weights (computed here on the CPU: it measures the
reference arithmetic, never the engine; 3x is the project's margin for accumulation-order
differences); the one-plan forward bit-equal to backbone + YolactHead as two calls."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet18_ref as rr
import yolact_head_ref as yr
from helpers import record_measurement
from recipe_yolact_head import head_case, head_inputs
from test_resnet18_cpu import BB, SMALL, small_config, small_desc
from tauv_vision_amd.weights import param_layout

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32x3", "fp16", "bf16"]
_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


# ---- the bandwidth kernels alone ----

@pytest.mark.parametrize("precision,C", [("fp32", 64), ("fp16", 8), ("fp16", 64), ("bf16", 64)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 6), (19, 26)])
def test_maxpool3x3s2_is_bit_equal_to_torch(H, W, C, precision):
    from tauv_vision_amd import _lib
    dt, B = _DT[precision], 2
    g = torch.Generator().manual_seed(100 * H + W + C)
    # negative everywhere: a zero-padded window would return 0 at every border pixel
    x = (-(torch.rand((B, H, W, C), generator=g) * 4 + 0.25)).to(dt)
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(dt)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(ref.shape) == (B, Ho, Wo, C)
    n, tail = ref.numel(), 64
    out = torch.full((n + tail,), float("nan"), dtype=dt).cuda()
    xd = x.cuda()
    _lib.check(_lib.lib().tv_diag_maxpool3x3s2(ctypes.c_void_p(xd.data_ptr()), B, H, W, C, ctypes.c_void_p(out.data_ptr()),
                                               _lib.DTYPES[precision], _lib.stream_of(xd.device)), "maxpool3x3s2")
    got = out.cpu()
    assert torch.isnan(got[n:]).all(), "wrote past the output"
    assert torch.equal(got[:n].reshape(ref.shape), ref)
    assert float(got[:n].float().max()) < 0


def test_maxpool3x3s2_refuses_partial_vectors():
    from tauv_vision_amd import _lib
    x, o = torch.zeros(1, 4, 4, 8).cuda(), torch.zeros(1, 2, 2, 8).cuda()
    for C, prec in ((6, "fp32"), (4, "fp16")):
        with pytest.raises(ValueError, match="16-byte"):
            _lib.check(_lib.lib().tv_diag_maxpool3x3s2(ctypes.c_void_p(x.data_ptr()), 1, 4, 4, C, ctypes.c_void_p(o.data_ptr()),
                                                       _lib.DTYPES[prec], _lib.stream_of(x.device)), "maxpool3x3s2")


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_add_relu_is_bit_equal_to_torch(precision):
    from tauv_vision_amd import _lib
    dt = _DT[precision]
    g = torch.Generator().manual_seed(21)
    a = torch.randn((2, 5, 7, 128), generator=g).to(dt)
    b = torch.randn((2, 5, 7, 128), generator=g).to(dt)
    ref = torch.relu(a.float() + b.float()).to(dt)
    n, tail = ref.numel(), 64
    out = torch.full((n + tail,), float("nan"), dtype=dt).cuda()
    ad, bd = a.cuda(), b.cuda()
    _lib.check(_lib.lib().tv_diag_add_relu(ctypes.c_void_p(ad.data_ptr()), ctypes.c_void_p(bd.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), n, _lib.DTYPES[precision],
                                           _lib.stream_of(ad.device)), "add_relu")
    got = out.cpu()
    assert torch.isnan(got[n:]).all(), "wrote past the output"
    assert torch.equal(got[:n].reshape(ref.shape), ref)
    assert 0.3 < float((got[:n] == 0).float().mean()) < 0.7  # both sides of the ReLU


# ---- the backbone against the float64 restatement ----

# [B, 3, H, W]: 37 gives an odd conv height (19), 51 an even conv width (26), the deepest map 2 x 2
SHAPES = [(2, 37, 51), (1, 64, 96), (3, 90, 160)]


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """(weights, image, float64 taps, per-tap error of the fp16 / bf16 emulation) of a case, once."""
    B, H, W = shape
    sd = rr.seeded_resnet18_state_dict(seed=H)
    g = torch.Generator().manual_seed(1000 + H)
    img = torch.randn((B, 3, H, W), generator=g)
    m = rr.resnet18_ref(sd)
    with torch.no_grad():
        ref = m(img.double())
        lowp = {}
        for p in ("fp16", "bf16"):
            low = m(img, lowp=_DT[p])
            lowp[p] = [float((a.double() - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(low, ref)]
    return sd, img, ref, lowp


def _backbone(sd, precision):
    from tauv_vision_amd.yolact import Resnet101Backbone
    bb = Resnet101Backbone(None, precision=precision)
    bb.load_state_dict({"_feature_extractor." + k: v for k, v in sd.items()}, strict=True)
    return bb


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_backbone_matches_float64_restatement(shape, precision):
    sd, img, ref, lowp = _reference(shape)
    taps = _backbone(sd, precision)(img.cuda())
    assert len(taps) == 3
    for i, (t, r) in enumerate(zip(taps, ref)):
        assert tuple(t.shape) == tuple(r.shape) and t.dtype == torch.float32
        t = t.cpu()
        assert torch.isfinite(t).all()
        rel = _rel(t, r)
        bound = 1e-4 if precision in ("fp32", "fp32x3") else 3 * lowp[precision][i]
        record_measurement(f"resnet18/{shape[1]}x{shape[2]}_b{shape[0]}/c{i + 3}/{precision}",
                           {"rel": rel, "bound": bound, "ratio": rel / bound, "ref_absmax": float(r.abs().max())})
        print(f"resnet18 {shape} c{i + 3} {precision}: rel {rel:.3e} bound {bound:.3e}")
        assert rel <= bound, f"{shape} c{i + 3} {precision}: {rel} > {bound}"


@pytest.mark.parametrize("shape", SHAPES)
def test_low_precision_bounds_have_teeth(shape):
    """On the CPU: the emulation's error is not zero, and a tap taken after the residual add or after
    the ReLU (not at bn2) is far outside every bound used above, on these inputs."""
    sd, img, ref, lowp = _reference(shape)
    m = rr.resnet18_ref(sd)
    for p in ("fp16", "bf16"):
        assert all(e > 0 for e in lowp[p])
    with torch.no_grad():
        for wrong in ("add", "relu"):
            for i, (w, r) in enumerate(zip(m(img.double(), tap=wrong), ref)):
                rel = _rel(w, r)
                assert rel > 3 * lowp["bf16"][i] and rel > 1e-4, f"{wrong} tap c{i + 3}: {rel}"


# ---- the whole model: one plan from the image ----

IMG_H, IMG_W = 72, 88  # -> 9x11, 5x6, 3x3 maps (head case A's sizes), levels 2x2 and 1x1


@functools.lru_cache(maxsize=None)
def _whole_weights():
    c = dict(head_case("yolact_head_a"), depths=(128, 256, 512))
    keys = [(k, s) for k, s in param_layout(small_desc(IMG_H, IMG_W)) if not k.startswith(BB)]
    head_sd, _ = head_inputs(c, layout=keys)
    bb_sd = rr.seeded_resnet18_state_dict(seed=9)
    return bb_sd, head_sd


def _yolact(precision):
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact
    bb_sd, head_sd = _whole_weights()
    cfg = small_config(IMG_H, IMG_W)
    net = Yolact(cfg, backbone=Resnet101Backbone(cfg, precision), precision=precision)
    full = {BB + k: v for k, v in bb_sd.items()}
    full.update(head_sd)
    net.load_state_dict(full, strict=True)
    return net


def _image(B, seed):
    return torch.randn((B, 3, IMG_H, IMG_W), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_plan_equals_backbone_then_head(precision):
    from tauv_vision_amd.yolact import YolactHead
    bb_sd, head_sd = _whole_weights()
    net = _yolact(precision)
    img = _image(2, 31)
    fused = net(img)
    taps = _backbone(bb_sd, precision)(img)
    assert [tuple(t.shape[1:]) for t in taps] == [(128, 9, 11), (256, 5, 6), (512, 3, 3)]
    head = YolactHead((128, 256, 512), small_config(IMG_H, IMG_W), precision=precision)
    head.load_state_dict(head_sd, strict=True)
    two = head(taps)
    names = ("classification", "box_encoding", "mask_coeff", "anchor", "mask_prototype")
    for name, a, b in zip(names, fused, two):
        assert a.shape == b.shape, name
        assert torch.equal(a, b), f"{name} {precision}: {float((a - b).abs().max())}"
    if precision != "fp32":
        return
    with torch.no_grad():
        ref_taps = rr.resnet18_ref(bb_sd)(img.cpu().double())
        hsd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in head_sd.items()}
        cls, enc, coef, proto, _ = yr.yolact_head(hsd, list(ref_taps), SMALL["C"], SMALL["k"])
    # (measured on MI355X: classification 1.1e-6, box_encoding 7.3e-7, mask_prototype 1.1e-6, mask_coeff 9.1e-5 —
    # its logits, of magnitude ~1e2 like the classification's, carry their fp32 error into tanh's (-1, 1) range,
    # where the bar's scale max(1, |ref|max) is 1)
    for name, got, ref in (("classification", fused[0], cls), ("box_encoding", fused[1], enc),
                           ("mask_coeff", fused[2], coef), ("mask_prototype", fused[4], proto)):
        rel = _rel(got.cpu(), ref)
        record_measurement(f"yolact_full/{name}/fp32", {"rel": rel})
        print(f"yolact_full {name}: rel {rel:.3e}")
        assert rel <= 1e-4, f"{name}: {rel}"


def test_batch_frames_match_single_frames():
    """B = 5 equals five single-frame calls and B = 17 (two concurrent slices, 9 + 8 frames, the image
    pointer advanced by its own frame size) its frames 0, 8 and 16, within the bound of the head's
    test_batch_slices_match_single_frames (the kernel choice, and so the order of the K sums, may
    depend on the batch); a repeat is bit-identical."""
    net = _yolact("fp16")
    for B, frames in ((5, range(5)), (17, (0, 8, 16))):
        img = _image(B, 40 + B)
        outs = [o.clone() for o in net(img)]
        for a, b in zip(net(img), outs):
            assert torch.equal(a, b)
        for i in frames:
            one = net(img[i:i + 1])
            for j in (0, 1, 2, 4):
                scale = max(1.0, float(outs[j].abs().max()))
                np.testing.assert_allclose(one[j].cpu().numpy(), outs[j][i:i + 1].cpu().numpy(), rtol=0, atol=1e-3 * scale)
    eng = next(iter(net._engines.values()))
    assert eng.slices(17) == [9, 8]


def test_graph_replay_of_out_form_is_bit_equal():
    net = _yolact("fp16")
    dev = torch.device("cuda", 0)
    B = 3
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        img = _image(B, 51)
        first = net(img)
        out = [torch.empty_like(first[0]), torch.empty_like(first[1]), torch.empty_like(first[2]),
               torch.empty((B, 4 * 9, 4 * 11, (SMALL["k"] + 3) // 4 * 4), device=dev)]
        res = net(img, out=out)  # the eager step on the capture stream: its workspaces exist before the capture
        assert res[0].data_ptr() == out[0].data_ptr() and res[4].data_ptr() == out[3].data_ptr()
        s.synchronize()
        eager = [o.clone() for o in out]
        for a, b in zip((first[0], first[1], first[2]), eager):
            assert torch.equal(a, b)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        net(img, out=out)
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(out, eager):
            assert torch.equal(o, e), "replayed outputs differ from the eager step"


def test_profile_multi_lists_the_new_kernels():
    net = _yolact("fp16")
    img = _image(2, 61)
    want = net(img)
    eng = next(iter(net._engines.values()))
    outs = [torch.empty_like(want[0]), torch.empty_like(want[1]), torch.empty_like(want[2]),
            torch.empty((2, 4 * 9, 4 * 11, 8), device=img.device)]
    rows = eng.profile_multi([img], outs)
    kernels = [r[3] for r in rows]
    assert sum(k.startswith("tv::rn::stem7s2_pool<") for k in kernels) == 1
    assert not any(k.startswith("tv::rn::maxpool3x3s2<") or k == "prep" for k in kernels)
    assert sum(k.startswith("tv::rn::add_relu<") for k in kernels) == 2
    assert not any(k.startswith("tv::nchw_to_nhwc<") or k.startswith("tv::rn::store_f32<") for k in kernels), \
        "the taps feed the lateral convs straight from the arena"
    labels = [r[0] for r in rows]
    assert not any("layer4.1 relu" in s for s in labels), "layer4.1's add and ReLU feed nothing"
    for a, b in zip(outs[:3], want[:3]):  # one op per launch, the same kernels: the same result
        assert torch.equal(a, b)
    # the backbone alone copies its three taps out; with the knob off (and in fp32) the stem and the
    # max-pool are launches of their own
    from tauv_vision_amd import engine as tv_engine
    for precision, knobs, fused in (("fp16", None, True), ("fp16", {"TV_RSTEM": "0"}, False), ("fp32", None, False)):
        tv_engine.set_diagnostic_knobs(knobs)
        try:
            bb = _backbone(_whole_weights()[0], precision)
            taps = bb.forward_nhwc(img)
        finally:
            tv_engine.set_diagnostic_knobs(None)
        beng = next(iter(bb._engines.values()))
        kernels = [r[3] for r in beng.profile_multi([img], [torch.empty_like(t) for t in taps])]
        assert sum(k.startswith("tv::rn::store_f32<") for k in kernels) == 3
        assert sum(k.startswith("tv::rn::add_relu<") for k in kernels) == 2
        assert sum(k.startswith("tv::rn::stem7s2_pool<") for k in kernels) == (1 if fused else 0)
        assert sum(k.startswith("tv::rn::maxpool3x3s2<") for k in kernels) == (0 if fused else 1)
        assert kernels.count("prep") == (0 if fused else 1)


def test_backbone_load_state_dict_rebuilds_the_engine():
    net = _yolact("fp32")
    img = _image(1, 71)
    before = net(img)[0].clone()
    eng = next(iter(net._engines.values()))
    assert next(iter(net._engines.values())) is eng
    other = {"_feature_extractor." + k: v for k, v in rr.seeded_resnet18_state_dict(seed=10).items()}
    net._backbone.load_state_dict(other, strict=True)
    after = net(img)[0]
    assert next(iter(net._engines.values())) is not eng, "a reload of the backbone must invalidate the engine"
    assert float((after - before).abs().max()) > 1e-3


def test_refusals_before_any_launch():
    net = _yolact("fp32")
    bb = net._backbone
    img = _image(2, 81)
    for m in (net, bb):
        with pytest.raises(ValueError, match="on cpu"):
            m(img.cpu())
        with pytest.raises(ValueError, match="expected img"):
            m(torch.zeros(2, 4, IMG_H, IMG_W).cuda())
    good = net(img)
    A, k = good[0].shape[1], SMALL["k"]
    ok = lambda: [torch.empty(2, A, SMALL["C"] + 1).cuda(), torch.empty(2, A, 4).cuda(), torch.empty(2, A, k).cuda(),
                  torch.empty(2, 36, 44, 8).cuda()]
    for i, bad in ((0, torch.empty(2, A + 1, SMALL["C"] + 1).cuda()), (3, torch.empty(2, 36, 44, 12).cuda()),
                   (1, torch.empty(1, A, 4).cuda())):
        out = ok()
        out[i] = bad
        with pytest.raises(ValueError, match="out"):
            net(img, out=out)
    with pytest.raises(ValueError, match="3 tensors"):
        bb(img, out=[torch.empty(2, 9, 11, 128).cuda()])
    with pytest.raises(ValueError, match="out"):
        bb(img, out=[torch.empty(2, 9, 11, 128).cuda(), torch.empty(2, 5, 6, 256).cuda(), torch.empty(2, 3, 3, 256).cuda()])
    res = net(img, out=ok())
    for a, b in zip(res[:3], good[:3]):
        assert torch.equal(a, b)
    # the single-pointer entry point refuses the several-output arch
    eng = next(iter(net._engines.values()))
    with pytest.raises(ValueError, match="4 output"):
        eng.forward(img)
    torch.cuda.synchronize()
