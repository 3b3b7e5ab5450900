"""tests/yolact_eval_ref.py (the float64 restatement the GPU tests compare against) and the package's
host-side average_precision, pinned to answers worked by hand. Needs no GPU and no library."""
import math

import numpy as np
import pytest

import yolact_eval_ref as ref
from tauv_vision_amd.yolact_evaluate import average_precision

# A hand-worked AP is a sum of 101 float64 samples divided by 101: its rounding error is below 101 ulps of
# a number <= 1, so the closed forms below hold to 101 * 2^-53 < 2e-14.
AP_TOL = 2e-14

TABLE = [([1, 0, 1], 2, (51 + 50 * 2 / 3) / 101), ([0, 1], 2, 25.5 / 101), ([1, 0, 0, 1, 1], 4, 56 / 101),
         ([1, 1], 2, 1.0), ([], 2, 0.0)]


def _log(flags, label=1, K=8, T=1):
    """One image's log: descending scores, the flags as box AND mask tp at every threshold."""
    log = np.zeros((1, K, 4), dtype=np.uint32)
    word = sum((1 << j) | (1 << (16 + j)) for j in range(T))
    for i, f in enumerate(flags):
        log[0, i, 0] = np.array([0.9 - 0.1 * i], dtype=np.float32).view(np.uint32)[0]
        log[0, i, 1] = label
        log[0, i, 2] = word if f else 0
        log[0, i, 3] = 1
    return log


@pytest.mark.parametrize("flags,n,want", TABLE)
def test_ap_table(flags, n, want):
    assert abs(ref.ap_of_flags(flags, n) - want) <= AP_TOL
    got = average_precision(_log(flags), [0, n], 1)
    assert got.ap.shape == (2, 1, 2)
    for kind in (0, 1):
        assert abs(got.ap[kind, 0, 1] - want) <= AP_TOL
        assert got.ap[kind, 0, 1] == ref.ap_of_flags(flags, n)  # the two are the same float
        assert math.isnan(got.ap[kind, 0, 0])
    assert got.n_detections == len(flags)


def test_a_class_without_truths_is_nan_and_left_out_of_map():
    log = np.concatenate([_log([1, 0, 1], label=1), _log([1, 1], label=2), _log([0, 1], label=3)])
    got = average_precision(log, [0, 2, 0, 2], 1)
    assert math.isnan(got.ap[0, 0, 2]) and math.isnan(got.ap[0, 0, 0])
    a, c = (51 + 50 * 2 / 3) / 101, 25.5 / 101
    assert abs(got.map[0] - (a + c) / 2) <= AP_TOL and abs(got.map[1] - (a + c) / 2) <= AP_TOL
    rap, rmap = ref.average_precision(log, [0, 2, 0, 2], 1)
    assert np.array_equal(got.ap, rap, equal_nan=True) and np.array_equal(got.map, rmap)


def test_ap50_ap75_columns_and_precision_recall():
    log = _log([1, 0, 1], T=10)
    got = average_precision(log, [0, 2], 10)
    assert abs(got.ap50[0] - (51 + 50 * 2 / 3) / 101) <= AP_TOL and abs(got.ap75[1] - (51 + 50 * 2 / 3) / 101) <= AP_TOL
    odd = average_precision(_log([1, 0, 1], T=3), [0, 2], 3, iou_thresholds=[0.3, 0.6, 0.9])
    assert math.isnan(odd.ap50[0]) and math.isnan(odd.ap75[0])
    assert got.precision_recall(0.75, 0, "box") == (0.5, 0.5)  # scores 0.9, 0.8 pass: one tp of two truths
    assert got.precision_recall(0.95, 3, "mask") == (1, 0.0)


def test_without_truths_raises():
    with pytest.raises(ZeroDivisionError):
        average_precision(_log([1]), [0, 0], 1)
    with pytest.raises(ZeroDivisionError):
        ref.average_precision(_log([1]), [0, 0], 1)


def test_nan_score_raises():
    log = _log([1, 0])
    log[0, 1, 0] = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]
    with pytest.raises(ValueError):
        average_precision(log, [0, 1], 1)


def _squares():
    """A 4 x 4 detection mask and a 4 x 4 truth two columns to the right of it, on an 8 x 12 image."""
    masks = np.zeros((1, 8, 12), dtype=bool)
    masks[0, 2:6, 2:6] = True
    seg = np.full((8, 12), 255, dtype=np.uint8)
    seg[2:6, 4:8] = 0
    return masks, seg


def test_mask_iou_of_two_offset_squares():
    masks, seg = _squares()
    inter, det_area, truth_area = ref.overlap(masks, 1, seg, np.array([True]))
    assert (int(inter[0, 0]), int(det_area[0]), int(truth_area[0])) == (8, 16, 16)
    assert ref.mask_iou(inter[0, 0], det_area[0], truth_area[0]) == 8 / 24
    assert ref.mask_iou(0, 0, 0) == 0.0


def test_invalid_pixels_leave_all_three_counts():
    masks, seg = _squares()
    seg[2:6, 5] = 254  # one column of the intersection and of the truth
    seg[2, 2] = 254    # one pixel of the detection outside the truth
    inter, det_area, truth_area = ref.overlap(masks, 1, seg, np.array([True]))
    assert (int(inter[0, 0]), int(det_area[0]), int(truth_area[0])) == (4, 11, 12)
    # a value < N whose truth is not valid is background; rows past the count give zeros
    inter, det_area, truth_area = ref.overlap(masks, 1, seg, np.array([False]))
    assert (int(inter[0, 0]), int(det_area[0]), int(truth_area[0])) == (0, 11, 0)
    inter, det_area, truth_area = ref.overlap(masks, 0, seg, np.array([True]))
    assert (int(inter[0, 0]), int(det_area[0]), int(truth_area[0])) == (0, 0, 12)


def test_box_iou_by_hand():
    assert ref.box_iou((0.5, 0.5, 0.25, 0.25), (0.5, 0.625, 0.25, 0.25)) == 1 / 3  # half overlap: 1/32 of 3/32
    assert ref.box_iou((0.5, 0.5, 0.25, 0.25), (0.5, 0.5, 0.25, 0.25)) == 1.0
    assert ref.box_iou((0.25, 0.25, 0.25, 0.25), (0.75, 0.75, 0.25, 0.25)) == 0.0
    assert ref.box_iou((0.5, 0.5, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0)) == 0.0  # an empty union


def _walk(conf, det_boxes, truth_boxes, labels, thr=(0.5,), valid=None):
    K, N = len(conf), len(labels)
    records = np.zeros((K, 8), dtype=np.float32)
    records[:, 4:8] = det_boxes
    zeros = np.zeros((K, N), dtype=np.int64)
    return ref.walk_image(np.asarray(conf, dtype=np.float32), records, K,
                          np.ones(N, dtype=bool) if valid is None else np.asarray(valid), np.asarray(labels),
                          np.asarray(truth_boxes, dtype=np.float32), zeros, np.zeros(K, dtype=np.int64),
                          np.zeros(N, dtype=np.int64), np.asarray(thr, dtype=np.float32))


def test_best_iou_against_first_match():
    # truth 0 overlaps detection 0 with IoU 0.6, truth 1 with IoU 1; detection 1 sits on truth 0 exactly.
    # First-match gives det 0 -> truth 0 and det 1 -> nothing at tau 0.5 ... best-IoU gives both a truth.
    t0, t1 = (0.5, 0.5, 0.5, 0.5), (0.5, 0.625, 0.5, 0.5)
    assert ref.box_iou(t1, t0) == 0.6
    det_truth, log = _walk([[0.1, 0.9], [0.1, 0.8]], [t1, t0], [t0, t1], [1, 1])
    assert det_truth[:, 0, 0].tolist() == [1, 0]
    assert (int(log[0, 2]) & 1, int(log[1, 2]) & 1) == (1, 1)


def test_tie_rules():
    t0, t1 = (0.5, 0.375, 0.5, 0.5), (0.5, 0.625, 0.5, 0.5)
    mid = (0.5, 0.5, 0.5, 0.5)  # the same IoU 0.6 with both truths: the lowest truth index wins
    assert ref.box_iou(mid, t0) == ref.box_iou(mid, t1) == 0.6
    det_truth, _ = _walk([[0.0, 0.7], [0.0, 0.7]], [mid, mid], [t0, t1], [1, 1])
    # equal scores: the lower record index walks first and takes truth 0, the other takes truth 1
    assert det_truth[:, 0, 0].tolist() == [0, 1]
    det_truth, _ = _walk([[0.0, 0.7], [0.0, 0.7]], [mid, t1], [t0, t1], [1, 1])
    assert det_truth[:, 0, 0].tolist() == [0, 1]
    # the label comes from the foreground columns only, the lowest index on a tie
    assert ref.label_score(np.array([0.9, 0.05, 0.05], dtype=np.float32)) == (1, np.float32(0.05))
    det_truth, log = _walk([[0.9, 0.05, 0.05]], [t0], [t0, t0], [2, 1])
    assert det_truth[0, 0, 0] == 1 and int(log[0, 1]) == 1
    # a truth with a label outside 1..C matches nothing
    det_truth, _ = _walk([[0.0, 0.7]], [t0], [t0], [2])
    assert det_truth[0, 0, 0] == -1


def test_nan_score_walks_last():
    t0 = (0.5, 0.5, 0.5, 0.5)
    det_truth, _ = _walk([[0.0, float("nan")], [0.0, 0.1]], [t0, t0], [t0], [1])
    assert det_truth[:, 0, 0].tolist() == [-1, 0]


SCENES = ref.SCENES


def test_the_limits_scene_keeps_its_gap_and_its_64_owner_strip():
    """The largest scene: its gap and its special cases are checked here, its full evaluation on the GPU side."""
    scene = ref.make_scene(**SCENES["limits"])
    assert ref.gap(scene) >= 1e-9
    assert scene["seg"][0, 1, :64].tolist() == list(range(64)) and scene["valid"][0].all()
    assert (scene["label"][0] >= 1).all() and (scene["label"][0] <= scene["confidence"].shape[2] - 1).all()
    _, _, truth_area = ref.overlap(scene["masks"][0, :1], 1, scene["seg"][0], scene["valid"][0])
    assert (truth_area > 0).all()
    assert not scene["valid"][1].all()  # image 1 keeps a seg value < N whose truth is not valid


def test_the_45x70_scene_has_an_image_without_a_valid_truth():
    scene = ref.make_scene(**SCENES["45x70"])
    res = ref.evaluate(scene)
    assert scene["counts"].tolist() == [6, 0, 3] and not scene["valid"][2].any() and scene["valid"][0].any()
    assert not res["inter"][2].any() and not res["truth_area"][2].any() and res["det_area"][2, :3].all()
    assert (res["det_truth"][2] == -1).all() and not res["log"][2, :, 2].any()


@pytest.mark.parametrize("name", [n for n in SCENES if n != "limits"])
def test_scenes_keep_their_gap_and_are_not_vacuous(name):
    scene = ref.make_scene(**SCENES[name])
    assert ref.gap(scene) >= 1e-9
    res = ref.evaluate(scene)
    assert res["n_bad"] == 0 and res["n_truth"].sum() > 0
    assert (res["det_truth"] >= 0).any() and (res["inter"] > 0).any()
    ap, mean = ref.average_precision(res["log"], res["n_truth"], len(scene["thr"]))
    got = average_precision(res["log"], res["n_truth"], len(scene["thr"]))
    assert np.array_equal(got.ap, ap, equal_nan=True) and np.array_equal(got.map, mean)
    assert 0 < mean[0] < 1 and 0 < mean[1] < 1
