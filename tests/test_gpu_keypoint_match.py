"""tv_match_keypoints (csrc/keypoints.hip) through DeviceKeypointDecoder on the planted scenes of
keypoint_match_ref.py, checked by its replay checker on the device's own records (why a replay and not
equality: that module's text), on both table routes (scene A: the LDS table; scenes B and D: 70 x 130
entries, past the 4096 kept in LDS, so the errors are computed inside the walk).

Bounds: the checker's TIE = 1e-9 and the 5 % cap on tied steps are keypoint_match_ref's. Where the
oracle itself has no tied step (scene A, seeds 1, 2, 3, 5) the device matching must equal the host
matching of decode_keypoints exactly. PnP (>= 6 matched keypoints) needs OpenCV, which the test
environment does not have: both routes call the same _solve_poses, and the comparisons of detection
lists replace it by a no-op for both."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import keypoint_match_ref as ref

pytestmark = pytest.mark.gpu

_SCENES = {}


def _scene(name, seed, **override):
    key = (name, seed, tuple(sorted(override.items())))
    if key not in _SCENES:
        _SCENES[key] = ref.make_scene(name, seed, **override)
    return _SCENES[key]


def _prediction(scene, pred=None):
    from tauv_vision_amd.centernet import Prediction
    pr = pred or scene.pred
    fields = {f: None for f in Prediction.__dataclass_fields__}
    for f in ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size", "offset", "depth"):
        fields[f] = getattr(pr, f).cuda()
    return Prediction(**fields)


def _model_config(scene):
    import tauv_vision_amd as tv
    return tv.ModelConfig([1], [1], 4 * scene.H, 4 * scene.W, 2, 1.0)


def _decoder(scene):
    import tauv_vision_amd as tv
    return tv.DeviceKeypointDecoder(scene.B, len(scene.slots), len(scene.owner), scene.H, scene.W, scene.K, scene.K_kp,
                                    ref.object_config(scene), torch.device("cuda", 0))


def _run(scene, pred=None, thr=None, kp_thr=None, dec=None):
    """KeypointRecords of host numpy arrays (copies) of one decoder call."""
    dec = dec or _decoder(scene)
    dec(pred or _prediction(scene), _model_config(scene), scene.thr if thr is None else thr,
        scene.kp_thr if kp_thr is None else kp_thr)
    host = dec.host()
    return type(host)(*[t.numpy().copy() for t in host])


def _check(scene, r):
    return ref.check_matching(r.records, r.counts, r.keypoint_records, r.keypoint_counts, scene.owner, scene.max_slots,
                              r.kp_det, r.slot_kp, r.n_matched)


EVENTS = {"A": ("multi", "none", "excluded"), "B": ("multi", "excluded"), "C": ("multi", "none"),
          "D": ("multi", "none", "excluded")}


@pytest.mark.parametrize("name,seed", [("A", 1), ("A", 2), ("A", 3), ("A", 5), ("A", 4), ("B", 1), ("B", 2), ("C", 1),
                                       ("D", 1)])
def test_matching_replays_on_the_planted_scenes(name, seed, monkeypatch):
    import tauv_vision_amd as tv
    tvd = sys.modules["tauv_vision_amd.decode"]  # (the package attribute `decode` is the function)
    scene = _scene(name, seed)
    r = _run(scene)
    obj, obj_n, kp, kp_n = ref.oracle_records(scene)
    assert np.array_equal(r.counts, obj_n) and np.array_equal(r.keypoint_counts, kp_n)
    stats = _check(scene, r)
    print(f"scene {name} seed {seed}: counts {r.counts.tolist()} / {r.keypoint_counts.tolist()}, {stats}")
    for event in EVENTS[name]:
        assert stats[event] > 0, event
    ref.assert_tie_cap(stats, f"device, scene {name} seed {seed}")
    o_stats = ref.check_matching(obj, obj_n, kp, kp_n, scene.owner, scene.max_slots, *ref.oracle_assignment(
        scene, (obj, obj_n, kp, kp_n)))
    ref.assert_tie_cap(o_stats, f"oracle, scene {name} seed {seed}")
    if name == "A" and seed in (1, 2, 3, 5):
        assert stats["tied"] == 0 and o_stats["tied"] == 0
        monkeypatch.setattr(tvd, "_solve_poses", lambda *a: None)
        oc, mc = ref.object_config(scene), _model_config(scene)
        want = tv.decode_keypoints(_prediction(scene), mc, oc, None, scene.K, scene.K_kp, scene.thr, scene.kp_thr, 0.0)
        got = tv.keypoint_detections_from_records(r.records, r.counts, r.keypoint_records, r.slot_kp, True, mc, oc, None)
        assert got == want
        assert np.array_equal(r.kp_det, ref.oracle_assignment(scene)[0])


def test_more_than_64_objects_per_image():
    """Scene B at an object threshold of 0.2: all 80 planted logits pass, so K = 70 objects are kept and
    the walking wave's lanes hold two objects each."""
    scene = _scene("B", 1)
    r = _run(scene, thr=0.2)
    assert r.counts.tolist() == [70, 70]
    stats = _check(scene, r)
    assert (r.kp_det >= 64).any(), "no keypoint went to an object of rank >= 64"
    ref.assert_tie_cap(stats, "device, scene B at 0.2")


def test_both_table_routes_agree():
    """The first 58 keypoints of scene B with K_kp = 58 (70 x 58 = 4060 entries: the LDS table) and with
    K_kp = 130 (computed inside the walk): the same records, so the same matching, element for element."""
    walk, table = _scene("B", 1), _scene("B", 1, K_kp=58)
    assert table.K * table.K_kp <= 4096 < walk.K * walk.K_kp
    a, b = _run(walk), _run(table)
    assert np.array_equal(a.keypoint_records[:, :58], b.keypoint_records, equal_nan=True) and (b.keypoint_counts == 58).all()
    assert np.array_equal(a.kp_det[:, :58], b.kp_det)
    _check(table, b)
    assert (b.kp_det >= 0).sum() > 58  # both images matched most of their keypoints


@pytest.mark.parametrize("name", ["A", "B"])
def test_nan_affinity_goes_to_the_first_candidate(name):
    scene = _scene(name, 1)
    base = _run(scene)
    b, k, _, _ = ref.multi_step(scene, (base.records, base.counts, base.keypoint_records, base.keypoint_counts),
                                base.kp_det)
    flat = int(base.keypoint_records[b, k, 7])
    lab, iy, ix = flat // (scene.H * scene.W), flat // scene.W % scene.H, flat % scene.W
    pred = _prediction(scene)
    pred.keypoint_affinity = pred.keypoint_affinity.clone()
    pred.keypoint_affinity[b, lab, 0, iy, ix] = float("nan")
    r = _run(scene, pred)
    assert np.isnan(r.keypoint_records[b, k, 8]) and r.kp_det[b, k] >= 0
    stats = _check(scene, r)  # (the checker requires the first candidate at the NaN step)
    assert stats["nan"] == 1


def test_zero_counts_give_all_minus_one():
    scene = _scene("A", 1)
    dec = _decoder(scene)
    for thr, kp_thr in ((2.0, scene.kp_thr), (scene.thr, 2.0)):
        dec.packed.fill_(0x5A)
        r = _run(scene, thr=thr, kp_thr=kp_thr, dec=dec)
        assert (r.counts == 0).all() if thr == 2.0 else (r.keypoint_counts == 0).all()
        assert (r.kp_det == -1).all() and (r.slot_kp == -1).all() and (r.n_matched == 0).all()
        _check(scene, r)


def test_strided_nhwc_views_equal_dense_tensors():
    """The prediction as the models return it: channel slices of one NHWC head tensor."""
    from tauv_vision_amd.centernet import prediction_from_nhwc
    scene = _scene("A", 2)
    oc = ref.object_config(scene)
    pr = scene.pred
    nhwc = torch.cat([pr.heatmap.permute(0, 2, 3, 1), pr.keypoint_heatmap.permute(0, 2, 3, 1),
                      pr.keypoint_affinity.permute(0, 3, 4, 1, 2).flatten(3), pr.size, pr.offset, pr.depth,
                      torch.zeros((scene.B, scene.H, scene.W, 3))], dim=3).cuda()
    view = prediction_from_nhwc(nhwc, oc)
    assert not view.heatmap.is_contiguous() and torch.equal(view.keypoint_affinity.cpu(), pr.keypoint_affinity)
    a, b = _run(scene), _run(scene, view)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)  # (columns a decode has no input for are NaN)


def test_second_call_leaves_no_stale_rows():
    first, second = _scene("A", 1), _scene("A", 3)
    dec = _decoder(first)
    _run(first, dec=dec)
    again = _run(second, dec=dec)
    fresh = _run(second)
    for x, y in zip(again, fresh):
        assert np.array_equal(x, y, equal_nan=True)
    # and from buffers full of another pattern: every element is written by every call
    dec.packed.fill_(0x5A)
    for x, y in zip(_run(second, dec=dec), fresh):
        assert np.array_equal(x, y, equal_nan=True)


def test_limits_are_refused_before_any_launch():
    import tauv_vision_amd as tv
    from tauv_vision_amd import _lib
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig("o", A(False, None), A(False, None), A(False, None), True, True,
                                             [(0.0, 0.0, 0.0)] * 33)])
    with pytest.raises(ValueError, match="33 keypoints"):
        tv.DeviceKeypointDecoder(1, 1, 33, 8, 8, 4, 4, oc, "cuda:0")
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4096, dtype=torch.int32, device=dev)
    out = torch.full((3, 64), 7, dtype=torch.int32, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    o = [ctypes.c_void_p(out[i].data_ptr()) for i in range(3)]
    for n_kp, slots, K, K_kp in ((1, 33, 2, 2), (1, 0, 2, 2), (1, 1, 257, 2), (1, 1, 2, 1025), (0, 1, 2, 2)):
        rc = _lib.lib().tv_match_keypoints(p, p, p, p, p, p, n_kp, slots, 1, K, K_kp, *o, _lib.stream_of(dev))
        assert rc == _lib.TV_EINVAL, (n_kp, slots, K, K_kp)
        with pytest.raises(ValueError):
            _lib.check(rc, "match_keypoints")
    torch.cuda.synchronize()
    assert (out == 7).all(), "a refused call wrote its outputs"


def test_decoder_refusals():
    import tauv_vision_amd as tv
    scene = _scene("C", 1)
    dec, mc = _decoder(scene), _model_config(scene)
    before = dec.packed.clone()
    pred = _prediction(scene)
    no_heads = _prediction(scene)
    no_heads.keypoint_heatmap = no_heads.keypoint_affinity = None
    with pytest.raises(ValueError, match="no keypoint heads"):
        dec(no_heads, mc, 0.5, 0.3)
    host = _prediction(scene)
    host.keypoint_affinity = host.keypoint_affinity.cpu()
    with pytest.raises(ValueError, match="keypoint_affinity is on cpu"):
        dec(host, mc, 0.5, 0.3)
    wrong = _prediction(scene)
    wrong.size = wrong.size[:, :-1]
    with pytest.raises(ValueError, match="size shape"):
        dec(wrong, mc, 0.5, 0.3)
    with pytest.raises(ValueError, match="heatmap shape"):
        _decoder(_scene("A", 1))(pred, mc, 0.5, 0.3)
    assert torch.equal(dec.packed, before), "a refused call launched"
    with pytest.raises(ValueError, match="must be on the GPU"):
        tv.decode_keypoints_records(scene.pred, mc, ref.object_config(scene), scene.K, scene.K_kp, 0.5, 0.3)
    with pytest.raises(ValueError, match="no keypoint heads"):
        tv.decode_keypoints_records(no_heads, mc, ref.object_config(scene), scene.K, scene.K_kp, 0.5, 0.3)


def test_records_api_and_detection_lists(monkeypatch):
    """decode_keypoints_records == the decoder's arrays; keypoint_detections_from_records ==
    decode_keypoints field by field on scene A, seed 1; and it runs the same _solve_poses (which asks for
    OpenCV once an object holds >= 6 keypoints, as decode_keypoints does)."""
    import tauv_vision_amd as tv
    tvd = sys.modules["tauv_vision_amd.decode"]  # (the package attribute `decode` is the function)
    scene = _scene("A", 1)
    oc, mc, pred = ref.object_config(scene), _model_config(scene), _prediction(scene)
    rec = tv.decode_keypoints_records(pred, mc, oc, scene.K, scene.K_kp, scene.thr, scene.kp_thr)
    for x, y in zip(rec, _run(scene)):
        assert isinstance(x, np.ndarray) and np.array_equal(x, y, equal_nan=True)
    assert int(rec.n_matched.max()) >= 6
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="solvePnP needs OpenCV"):
            tv.keypoint_detections_from_records(rec.records, rec.counts, rec.keypoint_records, rec.slot_kp, True, mc, oc,
                                                None)
    monkeypatch.setattr(tvd, "_solve_poses", lambda *a: None)
    want = tv.decode_keypoints(pred, mc, oc, None, scene.K, scene.K_kp, scene.thr, scene.kp_thr, 0.0)
    got = tv.keypoint_detections_from_records(rec.records, rec.counts, rec.keypoint_records, rec.slot_kp, True, mc, oc,
                                              None)
    assert [len(x) for x in got] == [len(x) for x in want] == rec.counts.tolist()
    for gi, wi in zip(got, want):
        for g, w in zip(gi, wi):
            for f in ("label", "score", "y", "x", "h", "w", "depth", "keypoints", "keypoint_scores",
                      "keypoint_affinities", "cam_t_object"):
                assert getattr(g, f) == getattr(w, f), f
    assert sum(k is not None for im in got for d in im for k in d.keypoints) == int(rec.n_matched.sum())
