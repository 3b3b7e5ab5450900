"""The YOLACT node's callback after the forward, as one call (yolact_node.py:128-143, 177-193):
detection_records (csrc/yolact.hip) against float64 torch, YolactDetector against the same public calls
made one by one and against the reference-shaped unbatched sequence, its graph replay, and Yolact.detect.

Bounds. The anchor index, the class id and the box are exact (copies and an argmax over distinct
logits). The two probabilities are within 1e-4 absolute of the float64 softmax: the project's standing
treatment of a device transcendental (head_scatter's tanhf, the DLA-34 sigmoid); measured on MI355X:
see DESIGN §11. Masks of the batched and the unbatched route within 1e-6, test_yolact.py's bound for that
comparison. Everything the detector does is compared bit for bit with the calls it is made of."""
import numpy as np
import pytest
import torch

from helpers import record_measurement
from recipe import seeded_u8_frames
from test_gpu_resnet18 import IMG_H, IMG_W, _yolact

pytestmark = pytest.mark.gpu

NAN = float("nan")
_SOFTMAX_ERR = {}  # largest softmax error per class count, collected over the parametrised cases


def _records_case(C1, seed):
    B, A, n_max = 3, 77, 16
    g = torch.Generator().manual_seed(seed)
    # every row a permutation of distinct multiples of 0.25: the argmax is unambiguous
    cls = torch.stack([(torch.randperm(C1, generator=g) - C1 // 2) * 0.25 for _ in range(B * A)]).view(B, A, C1).float()
    box = torch.rand((B, A, 4), generator=g)
    det = torch.stack([torch.randperm(A, generator=g)[:n_max] for _ in range(B)]).to(torch.int64)
    counts = torch.tensor([0, 5, 16], dtype=torch.int32)
    return cls, box, det, counts


def _records_ref(cls, box, det, counts):
    """float64: (records [B, n, 8], confidence [B, n, C1]), zero at and past counts[b]."""
    B, n = det.shape
    rec = torch.zeros((B, n, 8), dtype=torch.float64)
    conf = torch.zeros((B, n, cls.shape[2]), dtype=torch.float64)
    for b in range(B):
        for d in range(int(counts[b])):
            a = int(det[b, d])
            p = torch.softmax(cls[b, a].double(), dim=-1)
            k = int(torch.argmax(cls[b, a]))
            rec[b, d] = torch.cat([torch.tensor([a, k, float(p[k]), float(p[1:].max())], dtype=torch.float64),
                                   box[b, a].double()])
            conf[b, d] = p
    return rec, conf


@pytest.mark.parametrize("C1", [2, 5, 70])
def test_detection_records_match_float64(C1):
    import tauv_vision_amd as tv
    cls, box, det, counts = _records_case(C1, seed=100 + C1)
    ref, cref = _records_ref(cls, box, det, counts)
    out = torch.full((3, 16, 8), NAN).cuda()
    conf = torch.full((3, 16, C1), NAN).cuda()
    rec, cf = tv.detection_records(cls.cuda(), box.cuda(), det.cuda(), counts.cuda(), out=out, confidence_out=conf)
    assert rec.data_ptr() == out.data_ptr() and cf.data_ptr() == conf.data_ptr()
    rec, cf = rec.cpu(), cf.cpu()
    assert not torch.isnan(rec).any() and not torch.isnan(cf).any(), "a row was not written"
    for b in range(3):
        c = int(counts[b])
        assert (rec[b, c:] == 0).all() and (cf[b, c:] == 0).all(), "rows at and past counts[b] must be zero"
        assert torch.equal(rec[b, :c, 0].double(), ref[b, :c, 0]), "anchor index"
        assert torch.equal(rec[b, :c, 1].double(), ref[b, :c, 1]), "class id"
        assert torch.equal(rec[b, :c, 4:], box[b, det[b, :c]]), "the box is copied bit for bit"
    err = max(float((rec[..., 2:4].double() - ref[..., 2:4]).abs().max()), float((cf.double() - cref).abs().max()))
    _SOFTMAX_ERR[f"c{C1}"] = err
    record_measurement("yolact_frames/softmax", {"max_abs_err": max(_SOFTMAX_ERR.values()), "bound": 1e-4,
                                                 "per_case": dict(_SOFTMAX_ERR)})
    print(f"detection_records C+1 = {C1}: softmax max abs err {err:.3e}")
    assert err <= 1e-4
    assert float(ref[1, :5, 2].min()) > 0 and float(cref[2].sum(-1).min()) > 0.999  # the reference is a softmax
    # without the optional output, into a fresh buffer: the same records
    rec2, none = tv.detection_records(cls.cuda(), box.cuda(), det.cuda(), counts.cuda())
    assert none is None and torch.equal(rec2.cpu(), rec)


def test_detection_records_tie_takes_the_lower_column():
    import tauv_vision_amd as tv
    cls, box, det, counts = _records_case(5, seed=7)
    counts = torch.tensor([16, 16, 16], dtype=torch.int32)
    a = int(det[1, 3])
    cls[1, a] = torch.tensor([-1.0, 0.5, 2.25, 0.0, 2.25])  # columns 2 and 4 tie
    b = int(det[2, 0])
    cls[2, b] = torch.tensor([1.5, 1.5, -2.0, 0.25, 1.0])   # the background ties with column 1
    rec, _ = tv.detection_records(cls.cuda(), box.cuda(), det.cuda(), counts.cuda())
    rec = rec.cpu()
    assert rec[1, 3, 0] == a and rec[1, 3, 1] == 2
    assert rec[2, 0, 0] == b and rec[2, 0, 1] == 0
    p = torch.softmax(cls[2, b].double(), -1)
    assert abs(float(rec[2, 0, 2]) - float(p[0])) <= 1e-4 and abs(float(rec[2, 0, 3]) - float(p[1])) <= 1e-4


# ---- YolactDetector ----

TOP_K, IOU = 20, 0.5
CAMERA = (100.0, 110.0, 60.0, 45.0)


def _graded_yolact(precision):
    """test_gpu_resnet18's 72 x 88 model with its classification layer scaled by 1 / 64. The seeded head's
    logits reach +-180 (measured), so every anchor's softmax is exactly 0 or 1 and no confidence threshold
    keeps more than none and fewer than top_k of them; scaled, the logits lie within +-3 and the confidences
    are graded. Nothing else of the model changes; every comparison below is between routes of this one model."""
    net = _yolact(precision)
    sd = net.state_dict()
    for k in ("_prediction_head._classification_layer.weight", "_prediction_head._classification_layer.bias"):
        sd[k] = sd[k] / 64
    net.load_state_dict(sd, strict=True)
    return net


def _depth(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(300, 5000, (B, 90, 120), generator=g, dtype=torch.int32)
    d[torch.rand((B, 90, 120), generator=g) < 0.1] = 0  # holes in the depth image
    return d.to(torch.uint16)


def _threshold(net, frames):
    """A confidence threshold inside the widest gap among the 11 most confident anchors of image 0 (from
    the model's own classification): image 0 then keeps at least 1 and at most 10 < top_k detections."""
    cls = net.forward_frames(frames)[0][0].cpu()
    conf = torch.softmax(cls, -1)[:, 1:].max(-1).values.sort(descending=True).values[:11]
    gaps = conf[:-1] - conf[1:]
    j = int(torch.argmax(gaps))
    assert float(gaps[j]) > 1e-3, "the seeded model's confidences leave no usable gap"
    return float(conf[j] + conf[j + 1]) / 2


def _one_by_one(net, frames, thr, depth):
    """The detector's steps as separate public calls with fresh buffers."""
    import tauv_vision_amd as tv
    from tauv_vision_amd.yolact import BatchedNMS, assemble_masks_indexed, box_decode
    cls, enc, coef, anchor, proto = net.forward_frames(frames)
    box = box_decode(enc, anchor, net.config)
    B, A = cls.shape[:2]
    nms = BatchedNMS(B, A, TOP_K, frames.device)
    det, counts = nms(cls, box, IOU, thr)
    masks = assemble_masks_indexed(proto, coef, box, det, counts,
                                   out=torch.zeros((B, nms.K) + tuple(proto.shape[2:]), device=frames.device))
    rec, _ = tv.detection_records(cls, box, det, counts)
    pts = tv.DeviceLocalizer(B, nms.K, frames.device).masks(masks, counts, det, box, depth, *CAMERA, bound_by_box=True)
    return dict(cls=cls, box=box, coef=coef, proto=proto, det=det, counts=counts, masks=masks, records=rec, points=pts)


def _equal_detections(res, det, want, what):
    counts = want["counts"].cpu()
    assert torch.equal(res.counts.cpu(), counts), what
    assert torch.equal(res.records, want["records"]), what
    assert torch.equal(res.points, want["points"]), what
    for b in range(counts.shape[0]):
        c = int(counts[b])
        assert torch.equal(det[b, :c], want["det"][b, :c]), what
        assert torch.equal(res.masks[b, :c], want["masks"][b, :c]), what


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_detector_equals_its_steps_and_the_unbatched_sequence(precision):
    import tauv_vision_amd as tv
    from tauv_vision_amd.yolact import assemble_mask, box_decode, nms
    net = _graded_yolact(precision)
    dev = torch.device("cuda", 0)
    B = 2
    frames = seeded_u8_frames(B, IMG_H, IMG_W, seed=11).cuda()
    depth = _depth(B).cuda()
    thr = _threshold(net, frames)
    want = _one_by_one(net, frames, thr, depth)
    detector = tv.YolactDetector(net, B, (IMG_H, IMG_W), TOP_K, dev)
    res = detector(frames, IOU, thr, depth, CAMERA)
    counts = res.counts.cpu()
    print(f"detector {precision}: threshold {thr:.4f}, counts {counts.tolist()}")
    assert any(0 < int(c) < TOP_K for c in counts), counts
    assert detector.K == TOP_K and tuple(res.masks.shape) == (B, TOP_K, 36, 44)
    _equal_detections(res, detector.det, want, "detector vs its steps")
    for b in range(B):
        c = int(counts[b])
        assert (res.records[b, c:] == 0).all() and (res.points[b, c:] == 0).all()
        assert torch.equal(res.records[b, :c, 0].long(), detector.det[b, :c])
    # image 0 as the node computes it: box_decode -> nms -> assemble_mask -> localize_masks, unbatched
    cls, enc, coef, anchor, proto = net.forward_frames(frames)
    box = box_decode(enc, anchor, net.config)
    kept = nms(cls, box, TOP_K, IOU, thr)
    c0 = int(counts[0])
    assert torch.equal(kept, detector.det[0, :c0]), "kept indices of image 0"
    m0 = assemble_mask(proto[0], coef[0, kept], box[0, kept])
    np.testing.assert_allclose(res.masks[0, :c0].cpu().numpy(), m0.cpu().numpy(), rtol=0, atol=1e-6)
    p0 = tv.localize_masks(m0, kept, box[0], depth[:1], *CAMERA, bound_by_box=True)
    # (the region is mask > 0.5: the same pixels on both routes while no mask value is within the 1e-6 of 0.5)
    assert float((m0 - 0.5).abs().min()) > 1e-6
    assert np.array_equal(res.points[0, :c0].cpu().numpy(), p0)
    # the host copy, and Yolact.detect on the same frames
    rec, cnt, pts = detector.host()
    assert torch.equal(rec, res.records.cpu()) and torch.equal(cnt, counts) and torch.equal(pts, res.points.cpu())
    got = net.detect(frames, TOP_K, IOU, thr, depth.cpu().numpy(), CAMERA)
    assert torch.equal(got.records, rec) and torch.equal(got.counts, cnt) and torch.equal(got.points, pts)
    assert not got.records.is_cuda and got.masks.is_cuda
    for b in range(B):
        assert torch.equal(got.masks[b, :int(cnt[b])], res.masks[b, :int(cnt[b])])
    again = net.detect(frames, TOP_K, IOU, thr)
    assert again.points is None and torch.equal(again.records, rec)
    assert len(net._detectors) == 1
    net.invalidate()
    assert not net._detectors


def test_detector_graph_replay_is_bit_equal():
    import tauv_vision_amd as tv
    net = _graded_yolact("fp16")
    dev = torch.device("cuda", 0)
    B = 2
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        frames = seeded_u8_frames(B, IMG_H, IMG_W, seed=11).cuda()
        depth = _depth(B).cuda()
        thr = _threshold(net, frames)
        detector = tv.YolactDetector(net, B, (IMG_H, IMG_W), TOP_K, dev)
        detector(frames, IOU, thr, depth, CAMERA)  # the eager step on the capture stream
        s.synchronize()
        eager = dict(records=detector.records.clone(), points=detector.points.clone(), counts=detector.counts.clone(),
                     det=detector.det.clone(), masks=detector.masks.clone())
    torch.cuda.current_stream(dev).wait_stream(s)
    assert any(0 < int(c) < TOP_K for c in eager["counts"].cpu())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = detector(frames, IOU, thr, depth, CAMERA)
    for _ in range(3):
        for t in detector.head_out + [detector.box, detector.records, detector.masks, detector.points]:
            t.fill_(NAN)
        detector.counts.fill_(-1)
        detector.det.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _equal_detections(res, detector.det, eager, "replay vs the eager step")


def test_detect_resizes_frames_of_another_size():
    """Yolact.detect on 44 x 60 frames == YolactDetector fed preprocess(frames) through the fp32 entry."""
    import tauv_vision_amd as tv
    net = _graded_yolact("fp16")
    dev = torch.device("cuda", 0)
    B = 2
    frames = seeded_u8_frames(B, 44, 60, seed=13).cuda()
    img = tv.preprocess(frames, IMG_H, IMG_W)
    cls = net.forward(img)[0][0].cpu()
    conf = torch.softmax(cls, -1)[:, 1:].max(-1).values.sort(descending=True).values[:11]
    j = int(torch.argmax(conf[:-1] - conf[1:]))
    thr = float(conf[j] + conf[j + 1]) / 2
    detector = tv.YolactDetector(net, B, (IMG_H, IMG_W), TOP_K, dev)
    res = detector(img, IOU, thr)
    assert res.points is None
    rec, cnt, pts = detector.host()
    assert pts is None and int(cnt.max()) > 0
    got = net.detect(frames, TOP_K, IOU, thr)
    assert torch.equal(got.records, rec) and torch.equal(got.counts, cnt)
    for b in range(B):
        assert torch.equal(got.masks[b, :int(cnt[b])], detector.masks[b, :int(cnt[b])])
    # the cached detector of the camera size holds the static fp32 image the frames are resized into
    cached, = net._detectors.values()
    assert cached.frame_hw == (44, 60) and cached.size == (IMG_H, IMG_W) and torch.equal(cached.img, img)
