"""YOLACT from camera frames on the GPU: Resnet101Backbone.forward_frames / Yolact.forward_frames (uint8
NHWC frames, ToTensor + Normalize inside the plan's first kernel: stem7s2_pool's u8 instance in fp16 /
bf16, the staging kernel in fp32 / fp32x3 and with TV_RSTEM=0) against forward() of the reference image
recipe.normalize(frames.permute(0, 3, 1, 2).float() / 255) — the expression of the R18 test
(test_gpu_forward.py). Every comparison is bit for bit: the u8 entry stages exactly the values the fp32
entry rounds from that image, and everything after the staging is the same code.

Frames: recipe.seeded_u8_frames(2, H, W) with the first 256 pixels of frame 0 set to (v, v, v), v = 0..255,
so every (value, channel) entry of the LUT is read. Sizes: the stem test's (21, 33), (24, 36), (21, 36) —
one full and one partial 4 x 6 pooled tile in both axes, both parities of the conv size — and (22, 34);
their row strides of 99, 108, 108 and 102 bytes put the window rows at every byte alignment (99 mod 4 = 3
cycles through all four)."""
import functools

import pytest
import torch

import resnet18_ref as rr
from recipe import normalize, seeded_u8_frames
from test_gpu_resnet18 import IMG_H, IMG_W, _whole_weights, _yolact
from test_resnet18_cpu import SMALL, small_config

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32x3", "fp16", "bf16"]
SIZES = [(21, 33), (24, 36), (21, 36), (22, 34)]


def _frames(B, H, W, seed=0):
    f = seeded_u8_frames(B, H, W, seed=seed)
    if B:
        f[0].view(-1, 3)[:256] = torch.arange(256, dtype=torch.uint8)[:, None]
    return f


def _image(frames):
    # (contiguous NCHW: the permuted frames keep their NHWC strides through the arithmetic, and the engine's
    # op taps read the image through its raw pointer)
    return normalize(frames.permute(0, 3, 1, 2).float() / 255.0).contiguous()


@functools.lru_cache(maxsize=None)
def _bb_weights():
    return rr.seeded_resnet18_state_dict(seed=17)


def _backbone(precision):
    from tauv_vision_amd.yolact import Resnet101Backbone
    bb = Resnet101Backbone(None, precision=precision)
    bb.load_state_dict({"_feature_extractor." + k: v for k, v in _bb_weights().items()}, strict=True)
    return bb


def _with_knobs(knobs, fn):
    """fn() with the diagnostic knobs set: the engine a module builds on its first call reads them, and
    the module then keeps that engine for its later calls at the same size."""
    from tauv_vision_amd import engine as tv_engine
    tv_engine.set_diagnostic_knobs(knobs)
    try:
        return fn()
    finally:
        tv_engine.set_diagnostic_knobs(None)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        assert torch.isfinite(b).all(), (what, i)
        assert torch.equal(a, b), f"{what} output {i}: max diff {float((a - b).abs().max())}"


def test_the_frames_read_every_lut_entry():
    for H, W in SIZES:
        f = _frames(2, H, W)
        seen = torch.zeros(256, 3, dtype=torch.bool)
        for c in range(3):
            seen[f[..., c].reshape(-1).long(), c] = True
        assert seen.all(), (H, W)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W", SIZES)
def test_backbone_forward_frames_is_bit_equal_to_forward(H, W, precision):
    frames = _frames(2, H, W)
    img = _image(frames).cuda()
    fd = frames.cuda()
    for knobs in (None, {"TV_RSTEM": "0"}):
        bb = _backbone(precision)
        got = _with_knobs(knobs, lambda: bb.forward_frames(fd))
        want = bb.forward(img)
        _same(got, want, f"{H}x{W} {precision} {knobs}")
        eng = next(iter(bb._engines.values()))
        outs = [torch.empty_like(t.permute(0, 2, 3, 1)) for t in want]
        rows8 = eng.op_outputs_multi_u8(fd, outs)
        _same([o.permute(0, 3, 1, 2) for o in outs], want, "the u8 op tap")
        rows32 = eng.op_outputs_multi([img], outs)
        (_, k8, pool8), = [r for r in rows8 if r[0] == "maxpool"]
        (_, k32, pool32), = [r for r in rows32 if r[0] == "maxpool"]
        assert torch.equal(pool8, pool32), "the pooled tensors of the two entries differ"
        if precision in ("fp16", "bf16") and knobs is None:
            assert k8.startswith("tv::rn::stem7s2_pool<") and k8.endswith(", 1>"), k8
            assert k32.startswith("tv::rn::stem7s2_pool<") and k32.endswith(", 0>"), k32
            assert not any(r[1] == "prep" for r in rows8)
        else:
            assert k8.startswith("tv::rn::maxpool3x3s2<") and k32.startswith("tv::rn::maxpool3x3s2<"), (k8, k32)
            assert sum(r[1] == "prep" for r in rows8) == 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_unaligned_view_of_a_larger_batch(precision):
    """big[1:3] of 21 x 33 frames starts 2079 bytes into its allocation; the frame before and the frame
    after the batch hold 255, so an over-read that is used changes the result."""
    H, W = 21, 33
    frames = _frames(2, H, W)
    big = torch.full((4, H, W, 3), 255, dtype=torch.uint8)
    big[1:3] = frames
    big = big.cuda()
    view = big[1:3]
    assert view.is_contiguous() and view.data_ptr() % 4 == 3 and view.data_ptr() - big.data_ptr() == 2079
    bb = _backbone(precision)
    _same(bb.forward_frames(view), bb.forward(_image(frames).cuda()), f"view {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_yolact_forward_frames_is_bit_equal_to_forward(precision):
    net = _yolact(precision)
    frames = _frames(2, IMG_H, IMG_W, seed=3)
    got = net.forward_frames(frames.cuda())
    want = net.forward(_image(frames).cuda())
    assert len(got) == 5
    _same(got, want, f"yolact {precision}")
    assert got[4].shape[1] == SMALL["k"] and got[4].stride(1) == 1  # the NHWC view, as forward returns it


def test_yolact_forward_frames_in_two_slices():
    """B = 17 runs as slices of 9 + 8 frames: the second slice's frame pointer advances by H W 3 bytes."""
    net = _yolact("fp16")
    frames = _frames(17, IMG_H, IMG_W, seed=4)
    got = net.forward_frames(frames.cuda())
    want = net.forward(_image(frames).cuda())
    eng = next(iter(net._engines.values()))
    assert eng.slices(17) == [9, 8]
    for i in (0, 8, 16):
        for j in (0, 1, 2, 4):
            assert torch.equal(got[j][i], want[j][i]), (i, j)
    _same(got, want, "B = 17")


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_resize_path_is_preprocess_then_forward(precision):
    import tauv_vision_amd as tv
    frames = _frames(2, 30, 44, seed=5).cuda()
    bb = _backbone(precision)
    _same(bb.forward_frames(frames, size=(21, 33)), bb.forward(tv.preprocess(frames, 21, 33)), "backbone resize")
    net = _yolact(precision)
    big = _frames(2, 90, 120, seed=6).cuda()
    _same(net.forward_frames(big, size=(IMG_H, IMG_W)), net.forward(tv.preprocess(big, IMG_H, IMG_W)), "yolact resize")
    # a single frame [H, W, 3] is a batch of one
    _same(net.forward_frames(big[0], size=(IMG_H, IMG_W)), net.forward(tv.preprocess(big[:1], IMG_H, IMG_W)), "one frame")


def test_graph_replay_of_forward_frames_is_bit_equal():
    net = _yolact("fp16")
    dev = torch.device("cuda", 0)
    B = 3
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        frames = _frames(B, IMG_H, IMG_W, seed=7).cuda()
        first = net.forward_frames(frames)
        out = [torch.empty_like(first[0]), torch.empty_like(first[1]), torch.empty_like(first[2]),
               torch.empty((B, 4 * 9, 4 * 11, (SMALL["k"] + 3) // 4 * 4), device=dev)]
        res = net.forward_frames(frames, out=out)  # the eager step on the capture stream
        assert res[0].data_ptr() == out[0].data_ptr() and res[4].data_ptr() == out[3].data_ptr()
        s.synchronize()
        eager = [o.clone() for o in out]
        for a, b in zip((first[0], first[1], first[2]), eager):
            assert torch.equal(a, b)
        for a, b in zip(net.forward(_image(frames.cpu()).cuda())[:3], eager):
            assert torch.equal(a, b)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        net.forward_frames(frames, out=out)
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(out, eager):
            assert torch.equal(o, e), "replayed outputs differ from the eager step"


def test_empty_batch_behaves_as_forward_does():
    net = _yolact("fp16")
    frames = _frames(2, IMG_H, IMG_W)[:0].cuda()
    got = net.forward_frames(frames)
    want = net.forward(torch.zeros(0, 3, IMG_H, IMG_W).cuda())
    assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in want]
    assert got[0].shape[0] == 0 and [t.dtype for t in got] == [t.dtype for t in want]
    bb = net._backbone
    assert [tuple(t.shape) for t in bb.forward_frames(frames)] == \
        [tuple(t.shape) for t in bb.forward(torch.zeros(0, 3, IMG_H, IMG_W).cuda())]


def test_refusals_leave_the_outputs_untouched():
    from tauv_vision_amd.yolact import YolactHead
    net = _yolact("fp16")
    frames = _frames(2, IMG_H, IMG_W).cuda()
    good = net.forward_frames(frames)
    A, k = good[0].shape[1], SMALL["k"]
    nan = float("nan")

    def bufs():
        return [torch.full((2, A, SMALL["C"] + 1), nan).cuda(), torch.full((2, A, 4), nan).cuda(),
                torch.full((2, A, k), nan).cuda(), torch.full((2, 36, 44, 8), nan).cuda()]

    def untouched(out):
        torch.cuda.synchronize()
        assert all(torch.isnan(o).all() for o in out)

    # a head-only arch takes feature maps: the u8 entry refuses it before any launch
    _, head_sd = _whole_weights()
    head = YolactHead((128, 256, 512), small_config(IMG_H, IMG_W), precision="fp16")
    head.load_state_dict(head_sd, strict=True)
    heng = head.engine(frames.device, ((9, 11), (5, 6), (3, 3)))
    out = bufs()
    with pytest.raises(ValueError, match="not u8 frames"):
        heng.forward_multi_u8(frames, out)
    untouched(out)
    with pytest.raises(ValueError, match="not u8 frames"):
        heng.op_outputs_multi_u8(frames, out)
    untouched(out)
    for m in (net, net._backbone):
        out = bufs()
        with pytest.raises(ValueError, match="uint8"):  # an fp32 tensor passed as frames
            m.forward_frames(frames.float(), out=out)
        with pytest.raises(ValueError, match="uint8"):  # a last dimension that is not 3
            m.forward_frames(torch.zeros(2, IMG_H, IMG_W, 4, dtype=torch.uint8).cuda(), out=out)
        untouched(out)
    cpu_out = [o.cpu() for o in bufs()]
    with pytest.raises(ValueError, match="out"):
        net.forward_frames(frames, out=cpu_out)
    assert all(torch.isnan(o).all() for o in cpu_out)
    with pytest.raises(ValueError, match="out"):
        net._backbone.forward_frames(frames, out=[torch.full((2, 9, 11, 128), nan), torch.full((2, 5, 6, 256), nan),
                                                  torch.full((2, 3, 3, 512), nan)])
    res = net.forward_frames(frames, out=bufs())
    for a, b in zip(res[:3], good[:3]):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
