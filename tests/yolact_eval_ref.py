"""A float64 restatement, in plain loops, of the YOLACT evaluation's definitions (the contracts of
tv_yolact_mask_overlap and tv_yolact_evaluate_match in include/tauv_vision_amd.h, and average_precision's
docstring), written from those definitions and not from the kernels: the pixel counts from unpacked bool
masks, both IoUs, the walk, the log and the AP. Plus make_scene, a seeded synthetic scene with boxes on a
coarse grid (multiples of 1/16, exact in fp32, so every IoU is a ratio of small integers), and gap: the
smallest relative distance of any box IoU of a same-label pair to any threshold."""
import math

import numpy as np

INVALID = 254


def default_thresholds():
    import torch
    return torch.linspace(0.5, 0.95, 10).to(torch.float32).numpy()


# ---- counts -------------------------------------------------------------------------------------------

def overlap(masks, count, seg, valid):
    """masks [K, H, W] bool, seg [H, W] uint8, valid [N] bool -> inter [K, N], det_area [K], truth_area [N]."""
    K, N = masks.shape[0], valid.shape[0]
    inter = np.zeros((K, N), dtype=np.int64)
    det_area = np.zeros(K, dtype=np.int64)
    truth_area = np.zeros(N, dtype=np.int64)
    img_valid = seg != INVALID
    owner = [(seg == t) & img_valid if bool(valid[t]) and t != INVALID else None for t in range(N)]
    for t in range(N):
        if owner[t] is not None:
            truth_area[t] = int(owner[t].sum())
    for d in range(min(max(int(count), 0), K)):
        det_area[d] = int((masks[d] & img_valid).sum())
        for t in range(N):
            if owner[t] is not None:
                inter[d, t] = int((masks[d] & owner[t]).sum())
    return inter, det_area, truth_area


# ---- IoUs ---------------------------------------------------------------------------------------------

def box_iou(d, t):
    """d, t: (y, x, h, w) fp32 values; Python floats are doubles and Python never contracts."""
    yd, xd, hd, wd = (float(v) for v in d)
    yt, xt, ht, wt = (float(v) for v in t)
    y0d, y1d, x0d, x1d = yd - hd / 2, yd + hd / 2, xd - wd / 2, xd + wd / 2
    y0t, y1t, x0t, x1t = yt - ht / 2, yt + ht / 2, xt - wt / 2, xt + wt / 2
    ya = y0d if y0d > y0t else y0t
    yb = y1d if y1d < y1t else y1t
    xa = x0d if x0d > x0t else x0t
    xb = x1d if x1d < x1t else x1t
    sy, sx = yb - ya, xb - xa
    sy = sy if sy > 0.0 else 0.0
    sx = sx if sx > 0.0 else 0.0
    inter = sy * sx
    den = hd * wd + ht * wt - inter
    if den <= 0.0:
        return 0.0
    return inter / den


def mask_iou(inter, det_area, truth_area):
    union = int(det_area) + int(truth_area) - int(inter)
    return 0.0 if union == 0 else float(int(inter)) / float(union)


def label_score(row):
    """1 + argmax over the foreground columns of a softmax row [C + 1], the lowest index on a tie."""
    best, at = row[1], 1
    for c in range(2, len(row)):
        if row[c] > best:
            best, at = row[c], c
    return at, np.float32(best)


# ---- the walk -----------------------------------------------------------------------------------------

def walk_image(confidence, records, count, valid, label, box, inter, det_area, truth_area, thr):
    """One image -> det_truth [K, 2, T] int32, log [K, 4] uint32."""
    K, T, N = confidence.shape[0], len(thr), valid.shape[0]
    C = confidence.shape[1] - 1
    n = min(max(int(count), 0), K)
    det_truth = np.full((K, 2, T), -1, dtype=np.int32)
    log = np.zeros((K, 4), dtype=np.uint32)
    labels, scores = [], []
    for i in range(n):
        l, s = label_score(confidence[i])
        labels.append(l)
        scores.append(s)
    order = sorted(range(n), key=lambda i: (1, 0.0, i) if math.isnan(scores[i]) else (0, -float(scores[i]), i))
    usable = [bool(valid[t]) and 1 <= int(label[t]) <= C for t in range(N)]
    tp = [0] * n
    for kind in (0, 1):
        for j in range(T):
            tau = float(thr[j])
            free = list(usable)
            for i in order:
                best, best_iou = -1, 0.0
                for t in range(N):
                    if not free[t] or int(label[t]) != labels[i]:
                        continue
                    iou = box_iou(records[i, 4:8], box[t]) if kind == 0 else \
                        mask_iou(inter[i, t], det_area[i], truth_area[t])
                    if iou >= tau and (best < 0 or iou > best_iou):
                        best, best_iou = t, iou
                if best >= 0:
                    free[best] = False
                    det_truth[i, kind, j] = best
                    tp[i] |= 1 << (16 * kind + j)
    for i in range(n):
        log[i, 0] = np.array([scores[i]], dtype=np.float32).view(np.uint32)[0]
        log[i, 1] = labels[i]
        log[i, 2] = tp[i]
        log[i, 3] = 1
    return det_truth, log


def evaluate(scene):
    """The whole scene -> dict(inter, det_area, truth_area [int32], det_truth, log [B, K, 4] uint32, n_truth
    [C+1], n_bad)."""
    B, K = scene["masks"].shape[:2]
    N, C = scene["valid"].shape[1], scene["confidence"].shape[2] - 1
    out = dict(inter=[], det_area=[], truth_area=[], det_truth=[], log=[])
    n_truth, n_bad = np.zeros(C + 1, dtype=np.int64), 0
    for b in range(B):
        i, da, ta = overlap(scene["masks"][b], scene["counts"][b], scene["seg"][b], scene["valid"][b])
        dt, lg = walk_image(scene["confidence"][b], scene["records"][b], scene["counts"][b], scene["valid"][b],
                            scene["label"][b], scene["box"][b], i, da, ta, scene["thr"])
        for k, v in zip(("inter", "det_area", "truth_area", "det_truth", "log"), (i, da, ta, dt, lg)):
            out[k].append(v)
        for t in range(N):
            if scene["valid"][b, t]:
                if 1 <= int(scene["label"][b, t]) <= C:
                    n_truth[int(scene["label"][b, t])] += 1
                else:
                    n_bad += 1
    res = {k: np.stack(v) for k, v in out.items()}
    for k in ("inter", "det_area", "truth_area"):
        res[k] = res[k].astype(np.int32)
    res["n_truth"], res["n_bad"] = n_truth, n_bad
    return res


# ---- average precision --------------------------------------------------------------------------------

def ap_of_flags(flags, n_truth):
    """tp flags in score order, the class's truths -> the 101-point AP."""
    precision, recall = [], []
    ctp = cfp = 0.0
    for f in flags:
        if f:
            ctp += 1.0
        else:
            cfp += 1.0
        precision.append(ctp / (ctp + cfp))
        recall.append(ctp / float(n_truth))
    for i in range(len(precision) - 2, -1, -1):
        if precision[i + 1] > precision[i]:
            precision[i] = precision[i + 1]
    samples = []
    for r in np.linspace(0, 1, 101):
        at = 0
        while at < len(recall) and recall[at] < r:
            at += 1
        samples.append(precision[at] if at < len(recall) else 0.0)
    return float(np.mean(np.array(samples, dtype=np.float64)))


def average_precision(log, n_truth, T):
    """log [images, K, 4] uint32 -> (ap [2, T, C+1] with NaN for a class without truths, map [2])."""
    n_truth = [int(v) for v in n_truth]
    if sum(n_truth) == 0:
        raise ZeroDivisionError("division by zero")
    rows = []
    for r in np.asarray(log).view(np.uint32).reshape(-1, 4):
        if int(r[3]) == 1:
            rows.append((float(np.array([r[0]], dtype=np.uint32).view(np.float32)[0]), int(r[1]), int(r[2])))
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][0], i))
    ap = np.full((2, T, len(n_truth)), np.nan)
    for c in range(len(n_truth)):
        if n_truth[c] <= 0:
            continue
        for kind in (0, 1):
            for j in range(T):
                flags = [(rows[i][2] >> (16 * kind + j)) & 1 for i in order if rows[i][1] == c]
                ap[kind, j, c] = ap_of_flags(flags, n_truth[c])
    have = [c for c in range(len(n_truth)) if n_truth[c] > 0]
    mean = np.array([np.mean(np.array([[ap[kind, j, c] for c in have] for j in range(T)])) for kind in (0, 1)])
    return ap, mean


# ---- scenes -------------------------------------------------------------------------------------------

def _rect(H, W, box):
    """The pixel rectangle of a grid box (y, x, h, w in units of the image): rows y0..y1-1, columns x0..x1-1."""
    y, x, h, w = (float(v) for v in box)
    y0, y1 = int(round((y - h / 2) * H)), int(round((y + h / 2) * H))
    x0, x1 = int(round((x - w / 2) * W)), int(round((x + w / 2) * W))
    return max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)


def make_scene(seed, B, K, N, C, H, W, T=None, thr=None, counts=None, n_score_levels=6, rainbow=False,
               invalid_region=True, bad_value_truth=True, straddle=False, no_truth_image=None):
    """A seeded scene: truths as grid boxes painted into one seg map (lower index on top, so they are
    disjoint), detections as shifted copies of truths (mask and box shifted independently) or free boxes,
    scores from a few levels (equal scores are planted), records in random order. seg also holds a 254
    rectangle, 255 and other background values, and a value < N whose truth is not valid. `straddle`: truth
    0 also owns rows 6..10 x columns 60..67, across a strip border (x = 64) and a row-band border (y = 8),
    and detection 0's mask covers that region. `rainbow`: row 1 of image 0 starts with the 64 values 0..63 and
    all truths of that image are valid, so the 64 pixels of that strip have 64 different owners.
    `no_truth_image`: that image keeps its seg map and detections but has no valid truth."""
    rng = np.random.RandomState(seed)
    if thr is None:
        thr = default_thresholds() if T is None else np.linspace(0.3, 0.9, T).astype(np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    counts = np.asarray([K] * B if counts is None else counts, dtype=np.int32)
    masks = np.zeros((B, K, H, W), dtype=bool)
    seg = np.full((B, H, W), 255, dtype=np.uint8)
    valid = np.zeros((B, N), dtype=bool)
    label = np.zeros((B, N), dtype=np.int64)
    box = np.zeros((B, N, 4), dtype=np.float32)
    confidence = np.zeros((B, K, C + 1), dtype=np.float32)
    records = np.zeros((B, K, 8), dtype=np.float32)
    G = 16
    for b in range(B):
        seg[b, rng.randint(0, H, 8), rng.randint(0, W, 8)] = rng.randint(N, 254, 8) if N < 253 else 255
        for t in range(N):
            h, w = rng.randint(3, 9), rng.randint(3, 9)
            y, x = rng.randint(h // 2 + 1, G - h // 2), rng.randint(w // 2 + 1, G - w // 2)
            box[b, t] = (y / G, x / G, h / G, w / G)
            valid[b, t] = rng.rand() < 0.8
            label[b, t] = rng.randint(1, C + 1)
        if bad_value_truth and N > 1:
            valid[b, rng.randint(0, N)] = False  # its seg value stays in the map: background
        for t in range(N - 1, -1, -1):
            y0, y1, x0, x1 = _rect(H, W, box[b, t])
            seg[b, y0:y1, x0:x1] = t
        if invalid_region:
            y0, x0 = rng.randint(0, max(H - 4, 1)), rng.randint(0, max(W - 6, 1))
            seg[b, y0:y0 + 4, x0:x0 + 6] = INVALID
        if straddle:
            valid[b, 0] = True
            seg[b, 6:11, 60:68] = 0
        if rainbow and b == 0 and W >= 64:
            valid[b, :] = True
            seg[b, 1, :64] = np.arange(64) % N
            if W > 64:
                seg[b, 1, 64:] = (np.arange(W - 64) * 7) % N
        for d in range(K):
            for _attempt in range(100):  # redraw a detection whose box IoU with a truth sits on a threshold
                masks[b, d] = False
                t = rng.randint(0, N)
                if rng.rand() < 0.8:
                    by, bx, bh, bw = (float(v) * G for v in box[b, t])
                    dbox = ((by + rng.randint(-1, 2)) / G, (bx + rng.randint(-1, 2)) / G,
                            max(bh + rng.randint(-1, 2), 1) / G, max(bw + rng.randint(-1, 2), 1) / G)
                    lab = int(label[b, t]) if rng.rand() < 0.85 else rng.randint(1, C + 1)
                    y0, y1, x0, x1 = _rect(H, W, box[b, t])
                    sy, sx = rng.randint(-2, 3), rng.randint(-2, 3)
                    masks[b, d, max(y0 + sy, 0):max(y1 + sy, 0), max(x0 + sx, 0):max(x1 + sx, 0)] = True
                else:
                    h, w = rng.randint(2, 9), rng.randint(2, 9)
                    dbox = (rng.randint(2, G - 1) / G, rng.randint(2, G - 1) / G, h / G, w / G)
                    lab = rng.randint(1, C + 1)
                    y0, y1, x0, x1 = _rect(H, W, dbox)
                    masks[b, d, y0:y1, x0:x1] = True
                masks[b, d] ^= rng.rand(H, W) < 0.02
                score = (1 + rng.randint(0, n_score_levels)) / (n_score_levels + 2.0)
                row = rng.rand(C + 1).astype(np.float32) * np.float32(score * 0.5)
                row[lab] = np.float32(score)
                if C > 1 and rng.rand() < 0.2:  # a tie inside the row: the lowest index names the detection
                    row[rng.randint(1, C + 1)] = np.float32(score)
                row[0] = np.float32(rng.rand())  # the background column, often the largest: never a label
                confidence[b, d] = row
                records[b, d] = (rng.randint(0, 1000), int(np.argmax(row)), float(row.max()), score) + tuple(dbox)
                if all(abs(box_iou(records[b, d, 4:8], box[b, u]) - float(tau)) > 1e-6 * float(tau)
                       for u in range(N) for tau in thr):
                    break
            else:
                raise RuntimeError("make_scene: no detection box clear of the thresholds")
        if straddle:
            masks[b, 0, 5:12, 58:70] = True
    if no_truth_image is not None:
        valid[no_truth_image, :] = False
    return dict(masks=masks, counts=counts, seg=seg, valid=valid, label=label, box=box, confidence=confidence,
                records=records, thr=thr)


# the scenes of tests/test_gpu_yolact_evaluate.py, each reaching one path of the kernels; the CPU test checks
# their gap and that they are not vacuous
SCENES = {
    "45x70": dict(seed=1, B=3, K=6, N=3, C=3, H=45, W=70, counts=[6, 0, 3], no_truth_image=2),
    "64x65": dict(seed=2, B=2, K=6, N=3, C=2, H=64, W=65),
    "36x50": dict(seed=3, B=2, K=6, N=4, C=3, H=36, W=50),
    "k70": dict(seed=4, B=2, K=70, N=5, C=3, H=45, W=70, counts=[70, 65]),
    "limits": dict(seed=5, B=2, K=256, N=64, C=5, H=33, W=127, rainbow=True, counts=[256, 200]),
    "straddle": dict(seed=10, B=2, K=6, N=3, C=2, H=45, W=70, straddle=True),
    "t1": dict(seed=6, B=2, K=12, N=4, C=2, H=36, W=50, thr=[0.5]),
    "t16": dict(seed=7, B=2, K=12, N=4, C=2, H=36, W=50, T=16),
    "t16b": dict(seed=31, B=2, K=12, N=4, C=2, H=36, W=50, T=16),
    "t16c": dict(seed=32, B=2, K=12, N=4, C=2, H=36, W=50, T=16, counts=[12, 5]),
    "stream_a": dict(seed=8, B=3, K=12, N=5, C=3, H=45, W=70),
    "stream_b": dict(seed=9, B=2, K=12, N=3, C=3, H=45, W=70, counts=[12, 7]),
}


def gap(scene):
    """The smallest |IoU - tau| / tau over every same-label (detection, truth) pair's box IoU and every
    threshold (inf without such a pair)."""
    g = math.inf
    B, K = scene["masks"].shape[:2]
    for b in range(B):
        for d in range(min(int(scene["counts"][b]), K)):
            lab, _ = label_score(scene["confidence"][b, d])
            for t in range(scene["valid"].shape[1]):
                if scene["valid"][b, t] and int(scene["label"][b, t]) == lab:
                    iou = box_iou(scene["records"][b, d, 4:8], scene["box"][b, t])
                    for tau in scene["thr"]:
                        g = min(g, abs(iou - float(tau)) / float(tau))
    return g
