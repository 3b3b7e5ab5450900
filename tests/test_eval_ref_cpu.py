"""eval_ref.py against the reference itself: ONE walk over the records the reference's decode gives at the
lowest score threshold, counted per threshold, reproduces the (precision, recall) of the reference's own
evaluate_precision_recall run once per threshold (tests/golden/eval_*.npz, written by gen_golden_eval.py) —
equal as floats. That pins the prefix argument the device evaluation rests on. Then the walk's rules on
hand-made records."""
import os

import numpy as np
import pytest

import eval_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["eval_box_b3_l3_24x32", "eval_box_iou0_b3_l3_24x32", "eval_centre_b2_l1_24x32"]


def _scenes(g):
    """A scene per stored batch."""
    return [ref.scene_from_arrays(g["records"][i], g["counts"][i], g["valid"][i], g["label"][i], g["center"][i],
                                  g["size"][i], int(g["mode"]), float(g["match_threshold"]),
                                  score_thresholds=g["score_thresholds"]) for i in range(g["records"].shape[0])]


@pytest.mark.parametrize("name", CASES)
def test_one_walk_reproduces_the_reference_at_every_threshold(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    T = g["score_thresholds"].shape[0]
    assert T == 10
    n_tp, n_det, n_truth = np.zeros(T, np.int64), np.zeros(T, np.int64), 0
    for scene in _scenes(g):
        _, a, b, c = ref.evaluate_scene(scene)
        n_tp, n_det, n_truth = n_tp + a, n_det + b, n_truth + c
    precision, recall = ref.curve(n_tp, n_det, n_truth)
    print(name, n_tp.tolist(), n_det.tolist(), n_truth)
    assert precision == g["precision"].tolist()
    assert recall == g["recall"].tolist()
    assert len(set(n_det.tolist())) > 3 and n_tp[0] > n_tp[-1], "the thresholds do not cut the records apart"


@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert g["valid"].shape[2] - g["valid"].sum(axis=2).min() >= 1, "no invalid truth"
    for scene in _scenes(g):
        assert ref.gap(scene) >= 1e-6
        assert not ref.has_nan(scene)
        two_truths, two_records = ref.contention(scene)
        assert two_truths >= 1 and two_records >= 1


def _hand(records, valid, label, center, size, mode=ref.BOX, thr=0.5, thresholds=(0.0,), counts=None):
    records = np.asarray(records, dtype=np.float32)[None]
    counts = [records.shape[1]] if counts is None else counts
    return ref.scene_from_arrays(records, counts, [valid], [label], [center], None if size is None else [size], mode,
                                 thr, score_thresholds=thresholds)


BOXES = dict(valid=[True], label=[0], center=[(0.5, 0.5)], size=[(0.2, 0.2)])


def test_equal_scores_walk_the_later_record_first():
    rec = [(0, 0.5, 0.5, 0.5, 0.2, 0.2)] * 4  # four records, one truth
    assert ref.walk_order([0.5, 0.5, 0.5, 0.5]) == [3, 2, 1, 0]
    det, n_tp, n_det, n_truth = ref.evaluate_scene(_hand(rec, **BOXES))
    assert det.tolist() == [[-1, -1, -1, 0]] and (n_tp.tolist(), n_det.tolist(), n_truth) == ([1], [4], 1)
    # a higher score still goes first, wherever it stands
    rec[1] = (0, 0.75, 0.5, 0.5, 0.2, 0.2)
    assert ref.evaluate_scene(_hand(rec, **BOXES))[0].tolist() == [[-1, 0, -1, -1]]
    assert ref.walk_order([0.25, float("nan"), 0.5]) == [2, 0, 1]


def test_first_qualifying_truth_wins_not_the_best():
    # truth 0 overlaps the record a little (IoU 1/3 >= 0.3), truth 1 exactly: the record takes truth 0
    scene = _hand([(1, 0.9, 0.5, 0.5, 0.2, 0.2)], valid=[True, True], label=[1, 1],
                  center=[(0.5, 0.6), (0.5, 0.5)], size=[(0.2, 0.2), (0.2, 0.2)], thr=0.3)
    assert ref.evaluate_scene(scene)[0].tolist() == [[0]]
    # and a second record finds truth 0 gone and truth 1 still there
    scene = _hand([(1, 0.9, 0.5, 0.5, 0.2, 0.2), (1, 0.8, 0.5, 0.5, 0.2, 0.2)], valid=[True, True], label=[1, 1],
                  center=[(0.5, 0.6), (0.5, 0.5)], size=[(0.2, 0.2), (0.2, 0.2)], thr=0.3)
    assert ref.evaluate_scene(scene)[0].tolist() == [[0, 1]]


def test_invalid_truths_and_other_labels_are_never_taken():
    scene = _hand([(0, 0.9, 0.5, 0.5, 0.2, 0.2)], valid=[False, True, True], label=[0, 1, 0],
                  center=[(0.5, 0.5)] * 3, size=[(0.2, 0.2)] * 3)
    det, n_tp, n_det, n_truth = ref.evaluate_scene(scene)
    assert det.tolist() == [[2]] and n_truth == 2


def test_iou_threshold_zero_passes_disjoint_boxes_and_centre_mode_needs_no_size():
    far = [(0, 0.9, 0.1, 0.1, 0.05, 0.05)]
    assert ref.evaluate_scene(_hand(far, thr=0.0, **BOXES))[0].tolist() == [[0]]
    assert ref.evaluate_scene(_hand(far, thr=1e-9, **BOXES))[0].tolist() == [[-1]]
    near = dict(valid=[True], label=[0], center=[(0.5, 0.5)], size=None, mode=ref.CENTRE)
    assert ref.evaluate_scene(_hand([(0, 0.9, 0.5, 0.75, 0, 0)], thr=0.25, **near))[0].tolist() == [[0]]  # not >
    assert ref.evaluate_scene(_hand([(0, 0.9, 0.5, 0.76, 0, 0)], thr=0.25, **near))[0].tolist() == [[-1]]


def test_counts_over_thresholds_and_the_reference_formulas():
    rec = [(0, 0.75, 0.5, 0.5, 0.2, 0.2), (0, 0.5, 0.5, 0.5, 0.2, 0.2), (0, 0.25, 0.5, 0.5, 0.2, 0.2)]
    thresholds = (0.9, 0.5, 0.0)  # in any order; a score equal to a threshold counts
    det, n_tp, n_det, n_truth = ref.evaluate_scene(_hand(rec, thresholds=thresholds, **BOXES))
    assert (det.tolist(), n_tp.tolist(), n_det.tolist(), n_truth) == ([[0, -1, -1]], [0, 1, 1], [0, 2, 3], 1)
    assert ref.curve(n_tp, n_det, n_truth) == ([1, 0.5, 1 / 3], [0.0, 1.0, 1.0])  # no detection: precision 1
    assert ref.evaluate_scene(_hand(rec, thresholds=thresholds, counts=[2], **BOXES))[2].tolist() == [0, 2, 2]
    with pytest.raises(ZeroDivisionError):
        ref.precision_recall(0, 3, 0)
