"""The CenterNet node's callback as one call (centernet_node.py:90-178): CenternetDetector against the
same public calls made one by one (forward_frames -> DeviceKeypointDecoder -> DeviceLocalizer.boxes),
through the resize path and the fp32 entry, under graph replay, and model.detect_keypoints.

Everything the detector does is compared bit for bit with the calls it is made of: the same kernels on
the same inputs. Models: the smallest keypoint golden of CenterpointDLA34 (120 x 96) and a Centernet
with keypoint heads at 96 x 128, seeded weights, thresholds 0.05 (a seeded model's scores are low)."""
import numpy as np
import pytest
import torch

from recipe import seeded_u8_frames
from test_gpu_dla34 import build as build_dla34

pytestmark = pytest.mark.gpu

NAN = float("nan")
THR = KP_THR = 0.05
K, K_KP = 10, 50
CAMERA = (100.0, 110.0, 60.0, 45.0)


def _centernet(precision):
    import tauv_vision_amd as tv
    from tauv_vision_amd.weights import seeded_state_dict
    heights, channels, ds = [2] * 5, [16] * 6, 2
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), True, n > 0,
                                             [(0.1 * s, 0.0, 0.0) for s in range(n)] if n else None)
                             for i, n in enumerate([3, 0, 2])])
    model = tv.Centernet(tv.DLABackbone(heights, channels, ds), oc, precision=precision)
    model.load_state_dict(seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()]))
    return model.cuda().eval(), oc, tv.ModelConfig(heights, channels, 96, 128, ds, 1.0)


def _model(kind, precision):
    if kind == "dla34":
        model, oc, mc, _ = build_dla34("b1_120x96_kp", precision)
        return model, oc, mc
    return _centernet(precision)


def _depth(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(300, 5000, (B, 90, 120), generator=g, dtype=torch.int32)
    d[torch.rand((B, 90, 120), generator=g) < 0.1] = 0  # holes in the depth image
    return d.to(torch.uint16)


def _one_by_one(model, oc, mc, frames, depth):
    """The detector's steps as separate public calls with fresh buffers."""
    import tauv_vision_amd as tv
    pred = model.forward_frames(frames, (mc.in_h, mc.in_w))
    B, C, H, W = pred.heatmap.shape
    dec = tv.DeviceKeypointDecoder(B, C, oc.n_keypoints, H, W, K, K_KP, oc, frames.device)
    res = dec(pred, mc, THR, KP_THR)
    pts = tv.DeviceLocalizer(B, K, frames.device).boxes(res.records, res.counts, depth, *CAMERA)
    return pred, res, pts


def _same(a, b):
    """Bit for bit (record columns a decode has no input for are NaN, which torch.equal never finds equal)."""
    a, b = (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
    return torch.equal(a, b)


def _equal(res, want, pts, what):
    for f in res._fields[:-1]:
        assert _same(getattr(res, f), getattr(want, f)), f"{what}: {f}"
    assert _same(res.points, pts), f"{what}: points"


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("kind", ["dla34", "centernet"])
def test_detector_equals_its_steps(kind, precision):
    import tauv_vision_amd as tv
    model, oc, mc = _model(kind, precision)
    dev = torch.device("cuda", 0)
    B = 2
    frames = seeded_u8_frames(B, mc.in_h, mc.in_w, seed=11).cuda()
    depth = _depth(B).cuda()
    pred, want, pts = _one_by_one(model, oc, mc, frames, depth)
    det = tv.CenternetDetector(model, B, (mc.in_h, mc.in_w), mc, K, K_KP, dev)
    assert det.img is None
    res = det(frames, THR, KP_THR, depth, CAMERA)
    counts, kp_counts = res.counts.cpu(), res.keypoint_counts.cpu()
    print(f"detector {kind} {precision}: counts {counts.tolist()} / {kp_counts.tolist()}, matched "
          f"{int((res.kp_det >= 0).sum())}, valid points {int(res.points[..., 3].sum())}")
    assert int(counts.sum()) > 0 and int(kp_counts.sum()) > 0, "thresholds 0.05 leave nothing to decode"
    assert torch.equal(det.prediction.heatmap, pred.heatmap)
    assert torch.equal(det.prediction.keypoint_affinity, pred.keypoint_affinity)
    _equal(res, want, pts, "detector vs its steps")
    # the host copy, and detect_keypoints on the same frames
    host = det.host()
    for f in host._fields:
        assert not getattr(host, f).is_cuda and _same(getattr(host, f), getattr(res, f).cpu()), f
    got = model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR, depth.cpu().numpy(), CAMERA)
    for f in got._fields:
        assert _same(getattr(got, f), getattr(host, f)), f
    M = np.array([[CAMERA[0], 0.0, CAMERA[2]], [0.0, CAMERA[1], CAMERA[3]], [0.0, 0.0, 1.0]])
    by_matrix = model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR, depth.cpu(), M_projection=M)
    assert torch.equal(by_matrix.points, host.points)
    again = model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR)
    assert again.points is None and _same(again.records, host.records)
    assert torch.equal(again.slot_kp, host.slot_kp)
    # one cached detector, dropped with the parameters and rebuilt for another precision
    assert len(model._detectors) == 1
    cached, = model._detectors.values()
    model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR)
    assert next(iter(model._detectors.values())) is cached
    model.set_precision("bf16" if precision == "fp16" else "fp16")
    assert not model._detectors
    model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR)
    assert len(model._detectors) == 1 and next(iter(model._detectors.values())) is not cached
    model.load_state_dict(model.state_dict())
    assert not model._detectors


@pytest.mark.parametrize("kind", ["dla34", "centernet"])
def test_resize_path_and_fp32_entry(kind):
    """Frames of twice the model size: the detector preprocesses into its static fp32 image; the same
    image through the fp32 entry of a detector built at the model size gives the same buffers."""
    import tauv_vision_amd as tv
    model, oc, mc = _model(kind, "fp16")
    dev = torch.device("cuda", 0)
    B = 2
    frames = seeded_u8_frames(B, 2 * mc.in_h, 2 * mc.in_w, seed=13).cuda()
    depth = _depth(B).cuda()
    pred, want, pts = _one_by_one(model, oc, mc, frames, depth)
    det = tv.CenternetDetector(model, B, (2 * mc.in_h, 2 * mc.in_w), mc, K, K_KP, dev)
    res = det(frames, THR, KP_THR, depth, CAMERA)
    img = tv.preprocess(frames, mc.in_h, mc.in_w)
    assert torch.equal(det.img, img)
    assert int(res.counts.sum()) > 0 and int(res.keypoint_counts.sum()) > 0
    _equal(res, want, pts, "resize path vs its steps")
    entry = tv.CenternetDetector(model, B, (mc.in_h, mc.in_w), mc, K, K_KP, dev)
    assert entry.img is None
    _equal(entry(img, THR, KP_THR, depth, CAMERA), want, pts, "fp32 entry vs the resize path")
    got = model.detect_keypoints(frames, mc, K, K_KP, THR, KP_THR, depth.cpu(), CAMERA)
    cached, = model._detectors.values()
    assert cached.frame_hw == (2 * mc.in_h, 2 * mc.in_w) and cached.size == (mc.in_h, mc.in_w)
    assert _same(got.records, want.records.cpu()) and _same(got.points, pts.cpu())


def test_detector_graph_replay_is_bit_equal():
    import tauv_vision_amd as tv
    model, oc, mc = _model("centernet", "fp16")  # (its seeded weights give matches: 40 of 100 keypoints)
    dev = torch.device("cuda", 0)
    B = 2
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        frames = seeded_u8_frames(B, mc.in_h, mc.in_w, seed=11).cuda()
        other = seeded_u8_frames(B, mc.in_h, mc.in_w, seed=12).cuda()
        depth = _depth(B).cuda()
        det = tv.CenternetDetector(model, B, (mc.in_h, mc.in_w), mc, K, K_KP, dev)
        det(frames, THR, KP_THR, depth, CAMERA)  # the eager step on the capture stream
        s.synchronize()
        eager = det.decoder.packed.clone(), det.points.clone(), det.head_out.clone()
        det(other, THR, KP_THR, depth, CAMERA)
        s.synchronize()
        eager_other = det.decoder.packed.clone(), det.points.clone(), det.head_out.clone()
        static = frames.clone()
    torch.cuda.current_stream(dev).wait_stream(s)
    assert not torch.equal(eager[0], eager_other[0]), "the two frame sets decode to the same records"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        det(static, THR, KP_THR, depth, CAMERA)
    for src, want in ((frames, eager), (other, eager_other), (frames, eager)):
        static.copy_(src)
        det.head_out.fill_(NAN)
        det.points.fill_(NAN)
        det.decoder.packed.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(det.head_out, want[2])
        assert torch.equal(det.decoder.packed, want[0]), "replay vs the eager step: the decoder's buffers"
        assert torch.equal(det.points, want[1]), "replay vs the eager step: points"


def test_detector_refusals():
    import tauv_vision_amd as tv
    model, oc, mc = _model("centernet", "fp16")
    dev = torch.device("cuda", 0)
    A = tv.AngleConfig
    plain = tv.Centernet(tv.DLABackbone([2] * 5, [16] * 6, 2), tv.ObjectConfigSet(
        [tv.ObjectConfig("o", A(False, None), A(False, None), A(False, None), False, False, None)]))
    with pytest.raises(ValueError, match="keypoint heads"):
        tv.CenternetDetector(plain.cuda(), 1, (96, 128), mc, K, K_KP, dev)
    with pytest.raises(ValueError, match="CenterpointDLA34 or a Centernet"):
        tv.CenternetDetector(torch.nn.Linear(2, 2), 1, (96, 128), mc, K, K_KP, dev)
    with pytest.raises(ValueError, match="frame_hw"):
        tv.CenternetDetector(model, 0, (96, 128), mc, K, K_KP, dev)
    det = tv.CenternetDetector(model, 2, (96, 128), mc, K, K_KP, dev)
    before = det.decoder.packed.clone()
    frames = seeded_u8_frames(2, 96, 128, seed=3)
    depth = _depth(2).cuda()
    with pytest.raises(ValueError, match="tensor on cuda"):
        det(frames, THR, KP_THR)
    with pytest.raises(ValueError, match="built for"):
        det(frames[:1].cuda(), THR, KP_THR)
    with pytest.raises(ValueError, match="built for"):
        det(seeded_u8_frames(2, 48, 64, seed=3).cuda(), THR, KP_THR)
    with pytest.raises(ValueError, match="fp32 image"):
        det(torch.zeros((2, 3, 48, 64), device=dev), THR, KP_THR)
    with pytest.raises(ValueError, match="go together"):
        det(frames.cuda(), THR, KP_THR, depth)
    with pytest.raises(ValueError, match="depth"):
        det(frames.cuda(), THR, KP_THR, depth.cpu(), CAMERA)
    with pytest.raises(ValueError, match="depth"):
        det(frames.cuda(), THR, KP_THR, depth.float(), CAMERA)
    with pytest.raises(ValueError, match="fx and fy"):
        det(frames.cuda(), THR, KP_THR, depth, (0.0, 1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="goes with camera"):
        model.detect_keypoints(frames, mc, depth=depth.cpu())
    with pytest.raises(ValueError, match="uint8"):
        model.detect_keypoints(frames.float(), mc)
    torch.cuda.synchronize()
    assert torch.equal(det.decoder.packed, before), "a refused call launched"
