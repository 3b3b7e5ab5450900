"""tv_evaluate_detections (csrc/evaluate.hip) through DeviceEvaluator against eval_ref.py's float64
restatement on the same fp32 records: det_truth and every total EQUAL, on scenes that each reach one path
of the kernel; the reference's own ten (precision, recall) pairs of the three goldens through DeviceDecoder
+ DeviceEvaluator; and evaluate_precision_recall / _curve on a small model against the host.

Every scene asserts gap >= 1e-9 relative: no pair so close to the match threshold that a last-bit
difference between two correct double evaluations could show (there is none by construction: both sides
evaluate the same expressions in double)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_ref as ref
from helpers import case_by_name, case_input, case_state_dict

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def _evaluator(scene, B=None, N=None):
    import tauv_vision_amd as tv
    return tv.DeviceEvaluator(B or scene.B, scene.K, N or scene.N, scene.score_thresholds, scene.mode,
                              scene.match_threshold, DEV, columns=scene.columns, rec_stride=scene.rec_stride)


def _update(ev, scene):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return ev.update(t(scene.records), t(scene.counts), t(scene.valid), t(scene.label), t(scene.center),
                     t(scene.size))


def _device(scene, ev=None):
    ev = ev or _evaluator(scene)
    det = _update(ev, scene).cpu().numpy()
    tot = ev.totals.cpu().numpy()
    return det, tot[:ev.T], tot[ev.T:2 * ev.T], int(tot[2 * ev.T])


def _assert_equal(scene, got=None):
    assert ref.gap(scene, relative=True) >= 1e-9
    want = ref.evaluate_scene(scene)
    got = got or _device(scene)
    assert np.array_equal(got[0], want[0]), "det_truth"
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist() and got[3] == want[3]
    return want


SCENES = {
    "base": dict(K=8, N=3),
    "past_one_wave": dict(K=70, N=5),
    "past_one_thread_each": dict(K=300, N=9, B=3),
    "second_mask_word": dict(K=40, N=70, n_labels=1, spread=3.0),
    "ten_thresholds": dict(K=30, N=6, n_thresholds=10),
    "shuffled": dict(K=50, N=8, shuffle=True, n_thresholds=4),
    "iou_zero": dict(K=12, N=4, match_threshold=0.0, spread=40.0),
    "centre": dict(K=20, N=6, mode=ref.CENTRE, match_threshold=0.04),
    "yolact_layout": dict(K=16, N=5, rec_stride=8, columns=ref.YOLACT_COLUMNS),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_device_equals_the_float64_walk(name):
    scene = ref.make_scene(7, **SCENES[name])
    if name == "ten_thresholds":  # unsorted, one threshold equal to a planted score bit for bit
        thr = scene.score_thresholds[::-1].copy()
        thr[3] = scene.records[0, 5, 1]
        scene.score_thresholds = np.concatenate([thr[5:], thr[:5]])
    if name == "centre":
        scene.size = None  # truth_size = NULL
    if name == "second_mask_word":  # only truths past the first word can be taken: 64 is a copy of truth 0
        scene.label[:, :64] = 5
        scene.label[:, 64], scene.center[:, 64], scene.size[:, 64] = 0, scene.center[:, 0], scene.size[:, 0]
        scene.records[:, :2, 0] = 0
        scene.valid[:, 64] = True
    det, n_tp, n_det, _ = _assert_equal(scene)
    assert (det >= 0).any()
    if name == "second_mask_word":
        assert (det >= 64).any(), "no record took a truth of index >= 64"
    if name == "iou_zero":
        r, c = scene.records, scene.center
        assert any(det[b, k] >= 0 and ref.iou(*r[b, k, 2:6].tolist(), *c[b, det[b, k]].tolist(),
                                              *scene.size[b, det[b, k]].tolist()) == 0
                   for b in range(scene.B) for k in range(scene.K)), "no disjoint pair matched"
    if name == "ten_thresholds":
        assert len(set(n_det.tolist())) >= 5
    if name == "shuffled":
        s = ref.make_scene(7, **dict(SCENES[name], shuffle=False))
        assert not np.array_equal(s.records, scene.records)
        want = _assert_equal(s)
        assert (want[1].tolist(), want[2].tolist()) == (n_tp.tolist(), n_det.tolist())


def test_four_equal_scores_compete_for_one_truth():
    scene = ref.make_scene(3, B=1, K=6, N=1, n_labels=1, spread=0.1)
    scene.records[0, 1:5] = scene.records[0, 1]
    scene.records[0, 1:5, 0] = scene.label[0, 0]
    scene.records[0, 1:5, 2:4], scene.records[0, 1:5, 4:6] = scene.center[0, 0], scene.size[0, 0]
    scene.records[0, 0, 0] = 1  # the best score has another label
    det = _assert_equal(scene)[0]
    assert det.tolist() == [[-1, -1, -1, -1, 0, -1]]  # the last of the run walks first


def test_counts_of_zero_and_an_image_without_a_valid_truth():
    scene = ref.make_scene(5, B=3, K=10, N=4, counts=[0, 10, 7])
    scene.valid[2] = False
    det, n_tp, n_det, n_truth = _assert_equal(scene)
    assert (det[0] == -1).all() and (det[2] == -1).all() and n_det[0] == 17


def test_updates_accumulate_reset_restores_zero_and_no_stale_rows():
    a, b = ref.make_scene(1, B=2, K=12, N=4, n_thresholds=3), ref.make_scene(2, B=2, K=12, N=4, n_thresholds=3)
    b.score_thresholds = a.score_thresholds
    wa = ref.evaluate_scene(a)
    ev = _evaluator(a)
    _update(ev, a)
    ev.det_truth.fill_(0x5A5A5A5A)
    b.counts[:] = (5, 0)
    assert ref.gap(a, relative=True) >= 1e-9 and ref.gap(b, relative=True) >= 1e-9
    wb = ref.evaluate_scene(b)
    det = _update(ev, b).cpu().numpy()
    assert np.array_equal(det, wb[0]) and (det[0, 5:] == -1).all()
    tot = ev.totals.cpu().numpy()
    assert tot.tolist() == (wa[1] + wb[1]).tolist() + (wa[2] + wb[2]).tolist() + [wa[3] + wb[3]]
    r = ev.result()
    assert r.precision.tolist() == ref.curve(wa[1] + wb[1], wa[2] + wb[2], wa[3] + wb[3])[0] and r.n_truth == wa[3] + wb[3]
    ev.reset()
    assert (ev.totals == 0).all()
    with pytest.raises(ZeroDivisionError):
        ev.result()


def test_smaller_last_batch_fewer_truths_and_host_truths():
    scene = ref.make_scene(9, B=2, K=12, N=3)
    assert ref.gap(scene, relative=True) >= 1e-9
    want = ref.evaluate_scene(scene)
    ev = _evaluator(scene, B=4, N=7)
    assert np.array_equal(_update(ev, scene).cpu().numpy(), want[0])  # device truths: read as they are
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for buf in (ev.valid, ev.label, ev.center, ev.size, ev.det_truth):  # stale staging buffers and outputs
        buf.view(torch.uint8).fill_(0x5A)
    det = ev.update(t(scene.records).to(DEV), t(scene.counts).to(DEV), t(scene.valid), t(scene.label).int(),
                    t(scene.center), t(scene.size))  # host / int32 truths: staged, padded as invalid
    assert np.array_equal(det.cpu().numpy(), want[0])
    assert ev.totals.cpu().tolist() == [2 * int(want[1][0]), 2 * int(want[2][0]), 2 * want[3]]


def test_captured_graph_replays_equal_eager():
    scene = ref.make_scene(11, B=2, K=70, N=6, n_thresholds=5)
    want = _assert_equal(scene)
    ev = _evaluator(scene)
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
         for a in (scene.records, scene.counts, scene.valid, scene.label, scene.center, scene.size)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.update(*t)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(*t)
    for _ in range(2):
        ev.reset()
        ev.det_truth.fill_(7)
        graph.replay()
        tot = ev.totals.cpu().numpy()
        assert np.array_equal(ev.det_truth.cpu().numpy(), want[0])
        assert tot.tolist() == want[1].tolist() + want[2].tolist() + [want[3]]


def test_limits_are_refused_before_any_launch():
    import tauv_vision_amd as tv
    from tauv_vision_amd import _lib
    dev = torch.device(DEV)
    buf = torch.zeros(1 << 16, dtype=torch.int64, device=dev)
    out = torch.full((2, 4096), 7, dtype=torch.int64, device=dev)
    p, none = ctypes.c_void_p(buf.data_ptr()), None
    o = [ctypes.c_void_p(out[i].data_ptr()) for i in range(2)]
    good = (_lib.c_i32 * 6)(0, 1, 2, 3, 4, 5)
    bad = (_lib.c_i32 * 6)(0, 1, 2, 3, 4, 10)
    L, s = _lib.lib(), _lib.stream_of(dev)
    call = lambda K=8, N=3, T=1, cols=good, rec=p, size=p, mode=0: L.tv_evaluate_detections(
        rec, 10, p, cols, 1, K, p, p, p, size, N, mode, 0.5, p, T, o[0], o[1], s)
    for kw in (dict(K=1025), dict(N=257), dict(T=65), dict(cols=bad), dict(rec=none), dict(size=none), dict(mode=2),
               dict(N=0), dict(T=0)):
        rc = call(**kw)
        assert rc == _lib.TV_EINVAL, kw
        with pytest.raises(ValueError):
            _lib.check(rc, "evaluate_detections")
    assert call(K=0) == _lib.TV_OK  # launches nothing
    torch.cuda.synchronize()
    assert (out == 7).all(), "a refused call wrote its outputs"
    assert call(size=none, mode=1) == _lib.TV_OK  # centre mode takes no truth size
    for kw in (dict(K=1025), dict(N=257), dict(score_thresholds=[0.1] * 65), dict(columns=(0, 1, 2, 3, 4, 10))):
        args = dict(B=1, K=8, N=3, score_thresholds=[0.5], mode=0, match_threshold=0.5, device=DEV)
        with pytest.raises(ValueError):
            tv.DeviceEvaluator(**dict(args, **kw))
    scene = ref.make_scene(1)
    ev = _evaluator(scene)
    with pytest.raises(ValueError, match="on the GPU"):
        ev.update(torch.from_numpy(scene.records), torch.from_numpy(scene.counts).to(DEV), None, None, None, None)
    assert (ev.totals == 0).all()


# ---- the reference's own pairs ------------------------------------------------------------------------

def _prediction(g, i):
    from tauv_vision_amd.centernet import Prediction
    fields = {f: None for f in Prediction.__dataclass_fields__}
    fields.update(heatmap=torch.from_numpy(g["heatmap"][i]).to(DEV), size=torch.from_numpy(g["size_map"][i]).to(DEV),
                  offset=torch.from_numpy(g["offset"][i]).to(DEV))
    return Prediction(**fields)


@pytest.mark.parametrize("name", ["eval_box_b3_l3_24x32", "eval_box_iou0_b3_l3_24x32", "eval_centre_b2_l1_24x32"])
def test_goldens_reproduce_the_reference_curve(name):
    import tauv_vision_amd as tv
    from tauv_vision_amd.decode import DeviceDecoder
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    mode, thr = int(g["mode"]), g["score_thresholds"]
    nb, B, C, H, W = g["heatmap"].shape
    K, R = int(g["n_detections"]), 1 << int(g["downsamples"])
    dec = DeviceDecoder(B, C, H, W, K, DEV)
    ev = tv.DeviceEvaluator(B, K, g["valid"].shape[2], thr, mode, float(g["match_threshold"]), DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for i in range(nb):
        p = _prediction(g, i)
        rec, cnt = dec(p.heatmap, p.size, p.offset if mode == 0 else None, None, mode, R, int(g["in_h"]),
                       int(g["in_w"]), float(thr.min()))
        ev.update(rec, cnt, t(g["valid"][i]), t(g["label"][i]), t(g["center"][i]), t(g["size"][i]))
        assert cnt.cpu().tolist() == g["counts"][i].tolist()
    r = ev.result()
    assert r.precision.tolist() == g["precision"].tolist()
    assert r.recall.tolist() == g["recall"].tolist()


# ---- model level --------------------------------------------------------------------------------------

class _Batch:
    def __init__(self, img, valid, label, center, size):
        self.img, self.valid, self.label, self.center, self.size = img, valid, label, center, size

    def to(self, device):
        return _Batch(*[t.to(device) for t in (self.img, self.valid, self.label, self.center, self.size)])


class _Loader(list):
    passes = 0

    def __iter__(self):
        self.passes += 1
        return super().__iter__()


def _model():
    import tauv_vision_amd as tv
    name = "r18_c16_b2_96x128"
    case = case_by_name(name)
    o = case["objects"]
    A = tv.AngleConfig
    kp = o.get("keypoints_per_label", 0)
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(o.get("yaw", False), 1.0), A(o.get("pitch", False), 1.0),
                                             A(o.get("roll", False), 1.0), o.get("depth", False), kp > 0,
                                             [(0.0, 0.0, 0.0)] * kp if kp else None) for i in range(o["n_labels"])])
    model = tv.Centernet(tv.DLABackbone(case["heights"], case["channels"], case["downsamples"]), oc, precision="fp32")
    model.load_state_dict(case_state_dict(name))
    mc = tv.ModelConfig(case["heights"], case["channels"], case["in_h"], case["in_w"], case["downsamples"], 1.0)
    return model.cuda().eval(), mc, case_input(name)


def test_curve_equals_one_run_per_threshold_and_the_host():
    import tauv_vision_amd as tv
    model, mc, img = _model()
    imgs = [img, img.flip(-1), img.flip(-2)]
    N, iou_thr = 6, 0.3
    with torch.no_grad():
        decoded = [tv.decode_records(model(x.cuda()), mc, 100, 0.0) for x in imgs]
    scores = np.concatenate([r[..., 1].reshape(-1) for r, _ in decoded])
    thr = np.quantile(scores, [0.0, 0.3, 0.6, 0.9]).astype(np.float32)
    seed = 0
    while True:  # truths from the model's own decode at threshold 0, sizes jittered; re-drawn until the gap holds
        rng = np.random.default_rng(seed)
        batches, scenes = [], []
        for x, (rec, cnt) in zip(imgs, decoded):
            pick = np.stack([rng.choice(int(c), size=N, replace=False) for c in cnt])
            src = np.take_along_axis(rec, pick[..., None], axis=1)
            valid = rng.random(pick.shape) < 0.8
            size = (src[..., 4:6] * (0.6 + 0.8 * rng.random(src[..., 4:6].shape))).astype(np.float32)
            batches.append(_Batch(x, torch.from_numpy(valid), torch.from_numpy(src[..., 0].astype(np.int64)),
                                  torch.from_numpy(src[..., 2:4].copy()), torch.from_numpy(size)))
            scenes.append(ref.scene_from_arrays(rec, cnt, valid, src[..., 0], src[..., 2:4], size, ref.BOX, iou_thr,
                                                score_thresholds=thr))
        if min(ref.gap(s, relative=True) for s in scenes) >= 1e-9:
            break
        seed += 1
    loader = _Loader(batches)
    precision, recall = tv.evaluate_precision_recall_curve(model, mc, loader, DEV, iou_thr, score_thresholds=thr)
    assert loader.passes == 1, "the curve made more than one pass over the loader"
    singles = [tv.evaluate_precision_recall(model, mc, loader, DEV, float(t), iou_thr) for t in thr]
    assert precision.tolist() == [p for p, _ in singles] and recall.tolist() == [r for _, r in singles]
    tot = [sum(x) for x in zip(*[ref.evaluate_scene(s)[1:] for s in scenes])]
    assert tot[0][0] > 0 and tot[1][0] > tot[1][-1]
    assert (precision.tolist(), recall.tolist()) == ref.curve(*tot)
    assert tv.evaluate_precision_recall(model, mc, loader, DEV, float(thr[1]), iou_thr, max_batches=1) == \
        ref.precision_recall(*[x[1] if i < 2 else x for i, x in enumerate(ref.evaluate_scene(scenes[0])[1:])])
