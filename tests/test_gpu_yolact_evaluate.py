"""The YOLACT evaluation on the device (csrc/yolact_eval.hip, tauv_vision_amd/yolact_evaluate.py) against
tests/yolact_eval_ref.py, the float64 restatement that tests/test_yolact_eval_ref_cpu.py pins by hand. The
bits are synthetic, so the kernels and the restatement read the same data: every integer output, det_truth
and the log words are EQUAL, and the AP is equal as float64. Every scene asserts gap >= 1e-9 (no box IoU of
a same-label pair within 1e-9 relative of a threshold), which the scenes' coarse grid gives the restatement
alone."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yolact_eval_ref as ref
import tauv_vision_amd as tv
from tauv_vision_amd import _lib
from tauv_vision_amd.yolact import pack_frame_masks, unpack_frame_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _scene(name):
    scene = ref.make_scene(**ref.SCENES[name])
    assert ref.gap(scene) >= 1e-9
    return scene, ref.evaluate(scene)


def _bits(scene, garbage=False):
    """The packed bits of the scene's masks; `garbage`: every pad bit at x >= W set, and the rows at and past
    counts[b] filled with a pattern."""
    W = scene["masks"].shape[-1]
    bits = pack_frame_masks(torch.from_numpy(scene["masks"])).view(torch.int32).clone()
    if garbage:
        if W % 32:
            bits[..., -1] |= torch.tensor(-1 << (W % 32), dtype=torch.int64).to(torch.int32)
        for b, c in enumerate(scene["counts"]):
            bits[b, int(c):] = 0x5A5A5A5A
    return bits.view(torch.uint32).to(DEV)


def _inputs(scene, garbage=False):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(scene[k])).to(DEV)
    return (_bits(scene, garbage), t("counts"), t("confidence"), t("records"), t("seg"), t("valid"), t("label"),
            t("box"))


def _evaluator(scene, B=None, N=None, **kw):
    Bs, K, H, W = scene["masks"].shape
    return tv.DeviceYolactEvaluator(B or Bs, K, N or scene["valid"].shape[1], scene["confidence"].shape[2] - 1, (H, W),
                                    DEV, torch.from_numpy(scene["thr"]), **kw)


def _assert_batch(ev, want, what):
    for k in ("inter", "det_area", "truth_area", "det_truth"):
        got = getattr(ev, k).cpu().numpy()
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), f"{what}: {k}"


def _assert_state(ev, wants, what):
    """The cursor, totals and log rows against the restatement's results of the batches so far, in order."""
    cursor, totals, log = ev.host_state()
    want_log = np.concatenate([w["log"] for w in wants])
    assert cursor == want_log.shape[0], what
    assert np.array_equal(log[:cursor].view(np.uint32), want_log), f"{what}: log"
    assert not log[cursor:].any(), f"{what}: rows past the cursor"
    n_truth = sum(w["n_truth"] for w in wants)
    assert totals.tolist() == n_truth.tolist() + [sum(w["n_bad"] for w in wants)], f"{what}: totals"
    return want_log, n_truth


def _assert_ap(ev, want_log, n_truth, T):
    got = ev.result()
    ap, mean = ref.average_precision(want_log, n_truth, T)
    assert np.array_equal(got.ap, ap, equal_nan=True) and np.array_equal(got.map, mean)
    return got


@pytest.mark.parametrize("name", ["45x70", "64x65", "36x50", "k70", "limits", "straddle", "t1", "t16"])
def test_scene_equals_the_restatement(name):
    """45x70: W no multiple of 32 or 64, counts [K, 0, 3], an image of six bands; 64x65: one pixel into a
    second strip; 36x50: W < 64; k70: past one wave of keepers; limits: K = 256, N = 64 at 33 x 127, the
    16-byte fetch, and a seg row whose strip has 64 different owners; straddle: a truth across x = 64 and
    y = 8; t1 / t16: the threshold counts. Every scene holds 254 and 255, a value < N whose truth is not
    valid, unsorted records and equal scores. Garbage in the pad bits and in the rows past counts changes nothing."""
    scene, want = _scene(name)
    ev = _evaluator(scene)
    for garbage in (False, True):
        ev.reset()
        # a second update on outputs pre-filled with ones: every element is written by every call
        for buf in (ev._inter, ev._det_area, ev._truth_area, ev._det_truth):
            buf.fill_(1)
        ev.update(*_inputs(scene, garbage))
        _assert_batch(ev, want, f"{name} garbage={garbage}")
        want_log, n_truth = _assert_state(ev, [want], name)
    got = _assert_ap(ev, want_log, n_truth, len(scene["thr"]))
    assert got.n_detections == int(np.minimum(scene["counts"], scene["masks"].shape[1]).sum())
    if name == "limits":  # 64 different owners in one strip, each a valid truth: the peel loop runs 64 times
        assert scene["seg"][0, 1, :64].tolist() == list(range(64)) and scene["valid"][0].all()
        assert (want["truth_area"][0] > 0).all() and want["truth_area"].shape[1] == 64
    if name == "45x70":  # image 2 has detections and no valid truth
        assert scene["counts"].tolist() == [6, 0, 3] and not scene["valid"][2].any()
        assert not want["inter"][2].any() and not want["truth_area"][2].any() and want["det_area"][2, :3].all()
        assert (want["det_truth"][2] == -1).all() and (want["log"][2, :3, 3] == 1).all()
        assert not want["log"][2, :, 2].any()
    if name == "straddle":  # a truth across a strip border and a row-band border, on the word-by-word path
        assert (scene["seg"][0, 6:11, 60:68] == 0).all() and scene["valid"][0, 0] and want["inter"][0, 0, 0] >= 40


def test_two_batches_of_different_size_through_one_evaluator():
    (a, want_a), (b, want_b) = _scene("stream_a"), _scene("stream_b")
    ev = _evaluator(a)  # B = 3, N = 5; the second batch has 2 images of 3 truths
    ev.update(*_inputs(a))
    _assert_batch(ev, want_a, "first batch")
    ev.update(*_inputs(b), batch=2)
    _assert_batch(ev, want_b, "second batch")
    want_log, n_truth = _assert_state(ev, [want_a, want_b], "two batches")
    _assert_ap(ev, want_log, n_truth, len(a["thr"]))
    # host truths and fewer truths than N are staged; the answers are the same
    staged = _evaluator(a)
    args = _inputs(b)
    staged.update(*args[:5], *(torch.from_numpy(b[k]) for k in ("valid", "label", "box")), batch=2)
    assert np.array_equal(staged.det_truth.cpu().numpy(), want_b["det_truth"])
    assert np.array_equal(staged.inter.cpu().numpy()[:, :, :3], want_b["inter"])
    assert not staged.inter.cpu().numpy()[:, :, 3:].any()
    _assert_state(staged, [want_b], "staged truths")


def test_planted_equal_scores_and_equal_ious():
    scene = ref.make_scene(21, B=2, K=12, N=4, C=2, H=36, W=50, invalid_region=False, bad_value_truth=False)
    scene = {k: v.copy() for k, v in scene.items()}
    for b in range(2):
        # truths 0 and 1: one box and one label, so every detection has the same box IoU with both; their seg
        # regions are the two halves of the mask of detections 0 and 1, whose mask IoUs are equal too
        scene["box"][b, 1] = scene["box"][b, 0]
        scene["label"][b, :2] = 1
        scene["valid"][b, :2] = True
        scene["seg"][b] = 255
        scene["seg"][b, 10:20, 8:16] = 0
        scene["seg"][b, 10:20, 28:36] = 1
        scene["masks"][b, 0] = False
        scene["masks"][b, 0, 10:20, 8:16] = True   # exactly the two regions: IoU 80 / 160 with each truth,
        scene["masks"][b, 0, 10:20, 28:36] = True  # which passes the threshold 0.5 and no other
        scene["masks"][b, 1] = scene["masks"][b, 0]
        scene["confidence"][b, :2] = np.array([0.25, 0.75, 0.5], dtype=np.float32)  # equal scores, label 1
        scene["records"][b, :2, 4:8] = scene["box"][b, 0]
    assert ref.gap(scene) >= 1e-9
    want = ref.evaluate(scene)
    assert want["inter"][0, 0, 0] == want["inter"][0, 0, 1] == 80 and want["truth_area"][0, :2].tolist() == [80, 80]
    # the lowest truth index wins the equal IoUs; the second of the equal scores takes what is left
    assert want["det_truth"][0, 0, 0].tolist() == [0] * 10 and want["det_truth"][0, 1, 0].tolist() == [1] * 10
    assert want["det_truth"][0, :2, 1].tolist() == [[0] + [-1] * 9, [1] + [-1] * 9]
    ev = _evaluator(scene)
    ev.update(*_inputs(scene))
    _assert_batch(ev, want, "planted ties")
    want_log, n_truth = _assert_state(ev, [want], "planted ties")
    _assert_ap(ev, want_log, n_truth, 10)


def test_bad_label_nan_score_and_small_log_raise():
    scene, want = _scene("t1")
    C = scene["confidence"].shape[2] - 1
    bad = {k: v.copy() for k, v in scene.items()}
    b, t = np.argwhere(bad["valid"])[0]
    bad["label"][b, t] = C + 1
    ev = _evaluator(bad)
    ev.update(*_inputs(bad))
    assert ev.host_state()[1][C + 1] == 1
    with pytest.raises(ValueError, match="label"):
        ev.result()
    nan = {k: v.copy() for k, v in scene.items()}
    nan["confidence"][0, 0] = np.nan
    ev = _evaluator(nan)
    ev.update(*_inputs(nan))
    assert np.array_equal(ev.det_truth.cpu().numpy(), ref.evaluate(nan)["det_truth"])
    with pytest.raises(ValueError, match="NaN"):
        ev.result()
    # a log of one image with two guard rows behind it: the batch's second image is not written anywhere
    ev = _evaluator(scene, _capacity=1, _guard_rows=2)
    K = ev.K
    assert ev._state.numel() == ev._head + 3 * K * 4
    ev._state[ev._head + K * 4:] = 0x5A5A5A5A
    before = ev._state.clone()
    ev.update(*_inputs(scene))
    cursor, _, log = ev.host_state()
    assert cursor == 2 and np.array_equal(log[0].view(np.uint32), want["log"][0])
    assert torch.equal(ev._state[ev._head + K * 4:], before[ev._head + K * 4:]), "written past the log"
    with pytest.raises(ValueError, match="log holds"):
        ev.result()
    with pytest.raises(ValueError):
        ev.reserve(2)
    # the growing log: more images than the first capacity
    grow = _evaluator(scene)
    grow.capacity = 1
    grow._state = grow._new_state(1)
    for _ in range(3):
        grow.update(*_inputs(scene))
    assert grow.capacity >= 6
    _assert_state(grow, [want] * 3, "grown log")


def test_captured_graph_of_update_replayed_on_three_batches():
    names = ("t16", "t16b", "t16c")
    scenes = [_scene(n) for n in names]
    eager = _evaluator(scenes[0][0])
    for scene, _ in scenes:
        eager.update(*_inputs(scene, garbage=True))
    ev = _evaluator(scenes[0][0])
    ev.reserve(8)
    static = [t.clone() for t in _inputs(scenes[0][0])]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.update(*static)  # the eager step on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(*static)
    ev.reset()
    for scene, want in scenes:
        for dst, src in zip(static, _inputs(scene, garbage=True)):
            dst.copy_(src)
        graph.replay()
        _assert_batch(ev, want, "replay")
    _assert_state(ev, [w for _, w in scenes], "replays")
    a, b = eager.host_state(), ev.host_state()
    assert a[0] == b[0] == 6 and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:6], b[2][:6])
    assert np.array_equal(eager.result().ap, ev.result().ap, equal_nan=True)


def test_c_abi_argument_errors():
    dev = torch.device(DEV)
    buf = torch.zeros(1 << 16, dtype=torch.int64, device=dev)
    out = torch.full((1 << 16,), 7, dtype=torch.int64, device=dev)
    p, o = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr())
    L, s = _lib.lib(), _lib.stream_of(dev)

    def overlap(K=4, N=3, H=8, W=40, B=1, bits=p, inter=o):
        return L.tv_yolact_mask_overlap(bits, p, p, p, B, K, N, H, W, inter, o, o, s)

    def match(K=4, N=3, C=2, T=2, B=1, conf=p, cursor=o, capacity=4, log=o):
        return L.tv_yolact_evaluate_match(conf, p, p, p, p, p, p, p, p, p, B, K, N, C, T, cursor, log, capacity, o, o, s)

    for kw in (dict(K=0), dict(K=257), dict(N=0), dict(N=65), dict(H=0), dict(W=0), dict(B=0), dict(bits=None),
               dict(inter=None)):
        rc = overlap(**kw)
        assert rc == _lib.TV_EINVAL, kw
        with pytest.raises(ValueError):
            _lib.check(rc, "yolact_mask_overlap")
    for kw in (dict(K=0), dict(K=257), dict(N=0), dict(N=65), dict(C=0), dict(C=255), dict(T=0), dict(T=17), dict(B=0),
               dict(conf=None), dict(cursor=None), dict(capacity=-1), dict(log=ctypes.c_void_p(out.data_ptr() + 4))):
        assert match(**kw) == _lib.TV_EINVAL, kw
    torch.cuda.synchronize()
    assert (out == 7).all(), "a refused call wrote its outputs"
    for kw in (dict(K=257), dict(N=65), dict(n_classes=255), dict(iou_thresholds=[0.5] * 17), dict(B=0)):
        args = dict(B=1, K=4, N=3, n_classes=2, hw=(8, 40), device=DEV)
        args.update(kw)
        with pytest.raises(ValueError):
            tv.DeviceYolactEvaluator(**args)
    scene, _ = _scene("t1")
    ev = _evaluator(scene)
    args = list(_inputs(scene))
    with pytest.raises(ValueError):
        ev.update(args[0].cpu(), *args[1:])
    with pytest.raises(ValueError):
        ev.update(*args[:4], args[4][:, :-1].contiguous(), *args[5:])
    with pytest.raises(ValueError):
        ev.update(*args, batch=3)
    assert ev.host_state()[0] == 0


# ---- end to end on test_gpu_yolact_detect's 72 x 88 model ----

def _label_score(conf):
    fg = conf[:, 1:]
    return 1 + fg.argmax(1), fg.max(1)  # (numpy's argmax: the first index on a tie)


def test_evaluate_average_precision_end_to_end():
    from recipe import seeded_u8_frames
    from test_gpu_resnet18 import IMG_H, IMG_W
    from test_gpu_yolact_detect import IOU, TOP_K, _graded_yolact, _threshold
    H, W = IMG_H, IMG_W
    net = _graded_yolact("fp16")
    dev = torch.device(DEV)
    frames = seeded_u8_frames(5, H, W, seed=11).cuda()
    thr = _threshold(net, frames[:2])
    img = tv.preprocess(frames, H, W)

    def detect(x):
        """The package's detect path on one batch, copied to the host."""
        det = tv.YolactDetector(net, x.shape[0], (H, W), TOP_K, dev, frame_masks="bilinear")
        res = det(x, IOU, thr)
        conf = torch.zeros((x.shape[0], det.K, det.head_out[0].shape[2]), device=dev)
        tv.detection_records(det.head_out[0], det.box, det.det, det.counts, confidence_out=conf)
        return dict(masks=unpack_frame_masks(res.bits, W).cpu().numpy(), counts=res.counts.cpu().numpy(),
                    confidence=conf.cpu().numpy(), records=res.records.cpu().numpy())

    loader, scenes = [], []
    for lo, hi in ((0, 2), (2, 4), (4, 5)):  # three batches, the last one smaller
        x = img[lo:hi].contiguous()
        out = detect(x)
        Bn = hi - lo
        n = max(int(out["counts"].max() + 1) // 2, 1)
        assert n <= 64
        seg = np.full((Bn, H, W), 255, dtype=np.uint8)
        valid = np.zeros((Bn, n), dtype=bool)
        label = np.zeros((Bn, n), dtype=np.int64)
        box = np.zeros((Bn, n, 4), dtype=np.float32)
        for b in range(Bn):
            c = int(out["counts"][b])
            labels, scores = _label_score(out["confidence"][b, :c])
            chosen = list(range(0, c, 2))  # every other detection becomes a truth
            for t, d in enumerate(chosen):
                valid[b, t], label[b, t], box[b, t] = True, labels[d], out["records"][b, d, 4:8]
            for d in sorted(chosen, key=lambda d: -float(scores[d])):  # descending score: disjoint masks
                seg[b][out["masks"][b, d] & (seg[b] == 255)] = chosen.index(d)
        loader.append(SimpleNamespace(img=x.cpu(), seg=torch.from_numpy(seg), valid=torch.from_numpy(valid),
                                      classifications=torch.from_numpy(label), bounding_boxes=torch.from_numpy(box),
                                      img_valid=None))
        scenes.append(dict(out, seg=seg, valid=valid, label=label, box=box, thr=ref.default_thresholds()))
    got = tv.evaluate_average_precision(net, loader, dev, top_k=TOP_K, nms_iou_threshold=IOU, confidence_threshold=thr)
    wants = [ref.evaluate(s) for s in scenes]
    print("end to end: gap", min(ref.gap(s) for s in scenes), "counts", [s["counts"].tolist() for s in scenes])
    assert min(ref.gap(s) for s in scenes) >= 1e-9
    n_truth = sum(w["n_truth"] for w in wants)
    ap, mean = ref.average_precision(np.concatenate([w["log"] for w in wants]), n_truth, 10)
    print("end to end: map", got.map.tolist(), "ap50", got.ap50.tolist(), "n_truth", n_truth.tolist())
    assert np.array_equal(got.ap, ap, equal_nan=True) and np.array_equal(got.map, mean)
    assert got.n_truth.tolist() == n_truth.tolist() and got.n_detections == sum(int(s["counts"].sum()) for s in scenes)
    assert 0 < got.map[0] < 1 and 0 < got.map[1] < 1
    # max_batches stops early
    first = tv.evaluate_average_precision(net, loader, dev, top_k=TOP_K, nms_iou_threshold=IOU,
                                          confidence_threshold=thr, max_batches=1)
    assert first.n_detections == int(scenes[0]["counts"].sum())


def test_default_detector_is_the_sequence_of_its_public_calls():
    from recipe import seeded_u8_frames
    from test_gpu_resnet18 import IMG_H, IMG_W
    from test_gpu_yolact_detect import CAMERA, IOU, TOP_K, _depth, _equal_detections, _graded_yolact, _one_by_one, \
        _threshold
    net = _graded_yolact("fp16")
    frames = seeded_u8_frames(2, IMG_H, IMG_W, seed=11).cuda()
    thr, depth = _threshold(net, frames), _depth(2).cuda()
    detector = tv.YolactDetector(net, 2, (IMG_H, IMG_W), TOP_K, torch.device(DEV))
    res = detector(frames, IOU, thr, depth, CAMERA)
    assert detector.frame is None and res.bits is None and res.area is None and res.overlay is None
    _equal_detections(res, detector.det, _one_by_one(net, frames, thr, depth), "default detector vs its steps")
