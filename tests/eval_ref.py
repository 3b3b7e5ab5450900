"""Test infrastructure of the device evaluation (tv_evaluate_detections, csrc/evaluate.hip): a float64
restatement of the reference's detection-to-truth walk (centernet/scripts/evaluate.py:188-203 in box mode,
evaluate_keypoints.py:143-153 in centre mode) from record and truth arrays, the counts its precision and
recall are made of for a list of score thresholds, a seeded scene maker and the scene's distance from the
match threshold.

The reference runs the whole walk once per score threshold, on the records with score >= t. Those are a
prefix of the walk at the lowest threshold (descending score), and a record's match depends only on the
records walked before it, so ONE walk over all records gives every record its truth and n_tp(t),
n_detections(t) are counts over score >= t. test_eval_ref_cpu.py pins that against the reference's own
ten runs.

Arithmetic: the reference mixes Python floats (the detection) with fp32 0-d tensors (the truth), which
moves an IoU or a distance by about 1e-7 relative. Here, as on the device, the reference's expressions
are evaluated in double on the fp32 values, in the order written: Python floats do exactly that. The two
agree wherever no pair lies within that distance of the threshold, which `gap` measures.

A NaN score is outside the reference (a sigmoid gives none); here, as on the device, it walks last and
passes no threshold."""
from math import sqrt
from types import SimpleNamespace

import numpy as np

BOX, CENTRE = 0, 1
DECODE_COLUMNS = (0, 1, 2, 3, 4, 5)  # label, score, y, x, h, w of a tv_decode record
YOLACT_COLUMNS = (1, 3, 4, 5, 6, 7)  # ... of a tv_yolact_detection_records row


def iou(y1, x1, h1, w1, y2, x2, h2, w2):
    """evaluate.py:106-122 on Python floats (d1 the detection, d2 the truth)."""
    ya = max(y1 - h1 / 2, y2 - h2 / 2)
    xa = max(x1 - w1 / 2, x2 - w2 / 2)
    yb = min(y1 + h1 / 2, y2 + h2 / 2)
    xb = min(x1 + w1 / 2, x2 + w2 / 2)
    intersection = abs(max(yb - ya, 0) * max(xb - xa, 0))
    if intersection == 0:
        return 0.0
    a1 = w1 * h1
    a2 = w2 * h2
    return intersection / (a1 + a2 - intersection)


def distance(y1, x1, y2, x2):
    """evaluate_keypoints.py:66 (x ** 2 as x * x: the same double)."""
    dy, dx = y1 - y2, x1 - x2
    return sqrt(dy * dy + dx * dx)


def _passes(mode, d, t, thr):
    if mode == BOX:
        return iou(*d, *t) >= thr
    return not distance(d[0], d[1], t[0], t[1]) > thr


def _floats(row):
    return [float(v) for v in row]


def walk_order(scores):
    """reversed(sorted(range(n), key=score)): descending score, the later record first among equal scores;
    NaN last."""
    key = lambda i: (0, 0.0) if scores[i] != scores[i] else (1, float(scores[i]))
    return list(reversed(sorted(range(len(scores)), key=key)))


def walk(records, counts, columns, valid, label, center, size, mode, match_threshold):
    """det_truth [B, K] int32: the truth index each record took, or -1 (rows past counts[b]: -1)."""
    records = np.asarray(records, dtype=np.float32)
    B, K = records.shape[:2]
    cl, cs, cy, cx, ch, cw = columns
    N = np.asarray(valid).shape[1]
    det = np.full((B, K), -1, dtype=np.int32)
    thr = float(match_threshold)
    for b in range(B):
        n = int(min(max(int(counts[b]), 0), K))
        free = [m for m in range(N) if valid[b][m]]
        truth = {m: _floats((center[b][m][0], center[b][m][1]) +
                            ((size[b][m][0], size[b][m][1]) if size is not None else (0.0, 0.0))) for m in free}
        for i in walk_order(records[b, :n, cs]):
            r = records[b, i]
            d = _floats((r[cy], r[cx], r[ch], r[cw]))
            for m in free:
                if int(r[cl]) == int(label[b][m]) and _passes(mode, d, truth[m], thr):
                    det[b, i] = m
                    free.remove(m)
                    break
    return det


def totals(records, counts, columns, det_truth, valid, score_thresholds):
    """(n_tp [T], n_detections [T], n_truth) int64: counts over score >= t, compared in fp32."""
    records = np.asarray(records, dtype=np.float32)
    thr = np.asarray(score_thresholds, dtype=np.float32).reshape(-1)
    B, K = records.shape[:2]
    n_tp = np.zeros(thr.shape[0], dtype=np.int64)
    n_det = np.zeros(thr.shape[0], dtype=np.int64)
    for b in range(B):
        n = int(min(max(int(counts[b]), 0), K))
        s = records[b, :n, columns[1]]
        for t in range(thr.shape[0]):
            with np.errstate(invalid="ignore"):
                at = s >= thr[t]
            n_det[t] += int(at.sum())
            n_tp[t] += int((at & (det_truth[b, :n] >= 0)).sum())
    return n_tp, n_det, int(np.asarray(valid).astype(bool).sum())


def evaluate(records, counts, columns, valid, label, center, size, mode, match_threshold, score_thresholds):
    """(det_truth, n_tp, n_detections, n_truth) of one batch."""
    det = walk(records, counts, columns, valid, label, center, size, mode, match_threshold)
    return (det,) + totals(records, counts, columns, det, valid, score_thresholds)


def precision_recall(n_tp, n_detections, n_truth):
    """evaluate.py:205-206 on Python ints: ZeroDivisionError without a truth, as there."""
    n_tp, n_detections, n_truth = int(n_tp), int(n_detections), int(n_truth)
    precision = n_tp / n_detections if n_detections > 0 else 1
    recall = n_tp / n_truth
    return precision, recall


def curve(n_tp, n_detections, n_truth):
    pairs = [precision_recall(a, b, n_truth) for a, b in zip(n_tp, n_detections)]
    return [p for p, _ in pairs], [r for _, r in pairs]


def records_from_detections(detections, K=None):
    """decode()'s per-image Detection lists as decode-layout records [B, K, 6] fp32 and counts [B]. A
    Detection's floats came from fp32 records, so the way back is exact."""
    B = len(detections)
    K = K or max([len(d) for d in detections] + [1])
    rec = np.zeros((B, K, 6), dtype=np.float32)
    cnt = np.zeros((B,), dtype=np.int32)
    for b, dets in enumerate(detections):
        cnt[b] = len(dets)
        for k, d in enumerate(dets):
            rec[b, k] = (int(d.label), float(d.score), d.y, d.x, d.h, d.w)
    return rec, cnt


# ---- scenes ----------------------------------------------------------------------------------------

def make_scene(seed, B=2, K=8, N=3, n_labels=2, mode=BOX, match_threshold=0.3, n_thresholds=1, rec_stride=10,
               columns=DECODE_COLUMNS, counts=None, p_valid=0.85, shuffle=False, spread=0.5):
    """A seeded batch: truths in the unit square, and records planted around them (the same label for most,
    a centre within `spread` truth sizes, a size within +-30 %) so that many pairs lie on either side of the
    threshold. Truth 1 of every image is a near copy of truth 0 (a record qualifies for two truths) and
    records 0, 1 of every image sit on truth 0 (a truth wanted by two records). Scores are distinct fp32
    values, descending unless `shuffle`. Columns no role reads hold -7."""
    rng = np.random.default_rng(seed)
    valid = rng.random((B, N)) < p_valid
    label = rng.integers(0, n_labels, (B, N)).astype(np.int64)
    center = (0.1 + 0.8 * rng.random((B, N, 2))).astype(np.float32)
    size = (0.05 + 0.25 * rng.random((B, N, 2))).astype(np.float32)
    valid[:, 0] = True
    if N > 1:
        valid[:, 1] = True
        label[:, 1] = label[:, 0]
        center[:, 1] = center[:, 0] + (0.02 * size[:, 0]).astype(np.float32)
        size[:, 1] = size[:, 0]
    if counts is None:
        counts = np.full((B,), K, dtype=np.int32)
    counts = np.asarray(counts, dtype=np.int32)
    records = np.full((B, K, rec_stride), -7.0, dtype=np.float32)
    cl, cs, cy, cx, ch, cw = columns
    for b in range(B):
        scores = np.sort(rng.choice(np.arange(1, 1 << 20), size=K, replace=False))[::-1] / np.float32(1 << 20)
        for k in range(K):
            m = int(rng.integers(0, N)) if k >= 2 else 0
            same = rng.random() < 0.85 or k < 2
            jit = spread * (rng.random(2) - 0.5) * (0.2 if k < 2 else 2.0)
            records[b, k, cl] = label[b, m] if same else (label[b, m] + 1) % max(n_labels, 2)
            records[b, k, cs] = scores[k]
            records[b, k, cy] = center[b, m, 0] + jit[0] * size[b, m, 0]
            records[b, k, cx] = center[b, m, 1] + jit[1] * size[b, m, 1]
            records[b, k, ch] = size[b, m, 0] * (0.7 + 0.6 * rng.random())
            records[b, k, cw] = size[b, m, 1] * (0.7 + 0.6 * rng.random())
        if shuffle:
            records[b] = records[b, np.random.default_rng([seed, b]).permutation(K)]  # (rng's draws stay the same)
    lo = float(records[..., cs].min())
    thresholds = np.linspace(lo, 1.0, n_thresholds).astype(np.float32) if n_thresholds > 1 \
        else np.array([0.0], dtype=np.float32)
    return SimpleNamespace(B=B, K=K, N=N, mode=mode, match_threshold=float(match_threshold), columns=tuple(columns),
                           rec_stride=rec_stride, records=records, counts=counts, valid=valid, label=label,
                           center=center, size=size, score_thresholds=thresholds)


def _pairs(scene):
    """(b, record, truth, value) over the pairs the walk can test: same int label, a valid truth, a record
    before counts[b]; value the IoU (box) or the distance (centre) in double."""
    cl, cs, cy, cx, ch, cw = scene.columns
    for b in range(scene.B):
        n = int(min(max(int(scene.counts[b]), 0), scene.K))
        for i in range(n):
            r = scene.records[b, i]
            for m in range(scene.N):
                if not scene.valid[b][m] or int(r[cl]) != int(scene.label[b][m]):
                    continue
                t = _floats(scene.center[b][m])
                if scene.mode == BOX:
                    v = iou(*_floats((r[cy], r[cx], r[ch], r[cw])), *t, *_floats(scene.size[b][m]))
                else:
                    v = distance(float(r[cy]), float(r[cx]), *t)
                yield b, i, m, v


def gap(scene, relative=False):
    """The smallest |value - match_threshold| over the pairs the walk can test (relative: over the larger
    of the two magnitudes). A box pair at a threshold <= 0 is skipped: an IoU is the quotient of an abs()
    and a positive union, never negative in any arithmetic, so it passes whatever the rounding (the
    reference's iou_threshold = 0 quirk). inf without a pair."""
    thr, best = scene.match_threshold, float("inf")
    for _, _, _, v in _pairs(scene):
        if scene.mode == BOX and thr <= 0 and v >= 0:
            continue
        d = abs(v - thr)
        if relative:
            d /= max(abs(v), abs(thr), 1e-300)
        best = min(best, d)
    return best


def has_nan(scene):
    c = list(scene.columns) if scene.mode == BOX else list(scene.columns[:4])
    arrays = [scene.records[..., c], scene.center] + ([scene.size] if scene.size is not None else [])
    return any(bool(np.isnan(a).any()) for a in arrays)


def contention(scene):
    """(records that qualify for two or more truths, truths wanted by two or more records): what makes the
    walk order and the first-truth rule matter."""
    by_record, by_truth = {}, {}
    for b, i, m, v in _pairs(scene):
        ok = v >= scene.match_threshold if scene.mode == BOX else not v > scene.match_threshold
        if ok:
            by_record[(b, i)] = by_record.get((b, i), 0) + 1
            by_truth[(b, m)] = by_truth.get((b, m), 0) + 1
    return sum(c >= 2 for c in by_record.values()), sum(c >= 2 for c in by_truth.values())


def scene_from_arrays(records, counts, valid, label, center, size, mode, match_threshold, columns=DECODE_COLUMNS,
                      score_thresholds=(0.0,)):
    records = np.asarray(records, dtype=np.float32)
    valid = np.asarray(valid).astype(bool)
    return SimpleNamespace(B=records.shape[0], K=records.shape[1], N=valid.shape[1], mode=mode,
                           match_threshold=float(match_threshold), columns=tuple(columns),
                           rec_stride=records.shape[2], records=records, counts=np.asarray(counts, dtype=np.int32),
                           valid=valid, label=np.asarray(label, dtype=np.int64),
                           center=np.asarray(center, dtype=np.float32),
                           size=None if size is None else np.asarray(size, dtype=np.float32),
                           score_thresholds=np.asarray(score_thresholds, dtype=np.float32))


def evaluate_scene(scene):
    return evaluate(scene.records, scene.counts, scene.columns, scene.valid, scene.label, scene.center, scene.size,
                    scene.mode, scene.match_threshold, scene.score_thresholds)
