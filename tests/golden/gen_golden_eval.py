"""Golden fixtures for the device evaluation (reference centernet/scripts/evaluate.py:167-208 and
evaluate_keypoints.py:104-158).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's two evaluation scripts from
/root/reference/src with inert stand-ins for the modules their imports pull in and the evaluation never
needs (albumentations, cv2, spatialmath, torchvision.transforms.v2; matplotlib.pyplot, whose imshow /
show the keypoint script calls per image, as no-ops), and drives the reference's OWN
evaluate_precision_recall — once per score threshold, ten runs per case, as its
evaluate_precision_recall_curve does — with a fake model whose forward returns planted Predictions and a
list of fake batches. Stored per case as tests/golden/eval_*.npz: the planted predictions (without the keypoint
maps of the centre case, which no count depends on) and truths, the
reference's decode at the lowest threshold as records, the ten thresholds and the ten (precision, recall)
pairs. Data only: the reference source does not travel.
    python tests/golden/gen_golden_eval.py

Fixture conditions, asserted here and again by tests/test_eval_ref_cpu.py from the stored arrays: no pair
of equal labels within 1e-6 of the match threshold (the reference's mixed fp32 / double arithmetic moves
an IoU by about 1e-7), no NaN, at least one record that qualifies for two truths and one truth wanted by
two records. Asserted here only (they make the fixture independent of how a decode breaks ties and rounds
a sigmoid): the peak scores of every image at or above the lowest threshold, and the first below it, differ
pairwise by more than 2e-6 relative (of the 101 largest), and no
score lies within 1e-6 of a score threshold unless it equals it.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF_SRC = "/root/reference/src"
K = 100  # the scripts' decode(prediction, model_config, 100, ...)
H, W, DOWNSAMPLES = 24, 32, 2


def _import_reference():
    sys.dont_write_bytecode = True
    stubs = {n: types.ModuleType(n) for n in ("cv2", "spatialmath", "albumentations", "torchvision",
                                              "torchvision.transforms", "torchvision.transforms.v2",
                                              "matplotlib", "matplotlib.pyplot")}
    stubs["spatialmath"].SE3 = object
    stubs["spatialmath"].SO3 = object
    stubs["torchvision"].transforms = stubs["torchvision.transforms"]
    stubs["torchvision.transforms"].v2 = stubs["torchvision.transforms.v2"]
    stubs["matplotlib"].pyplot = stubs["matplotlib.pyplot"]
    for f in ("imshow", "show", "figure", "plot", "xlabel", "ylabel", "xlim", "ylim", "grid"):
        setattr(stubs["matplotlib.pyplot"], f, lambda *a, **k: None)
    for name, mod in stubs.items():
        sys.modules.setdefault(name, mod)
    # the keypoint script calls plt.imshow / plt.show for every image: pyplot is the stand-in even where a
    # real matplotlib is installed
    sys.modules["matplotlib.pyplot"] = stubs["matplotlib.pyplot"]
    sys.path.insert(0, REF_SRC)
    from tauv_vision.centernet.model import centernet as rnet
    from tauv_vision.centernet.model import config as rcfg
    from tauv_vision.centernet.model import decode as rdec
    from tauv_vision.centernet.scripts import evaluate as rbox
    from tauv_vision.centernet.scripts import evaluate_keypoints as rkp
    # evaluate_keypoints.py:86 builds its truths without KeypointDetection's w, h and depth, which the class
    # (decode.py:32-48) has no defaults for: the script fails there as it stands. The truths' w, h and depth
    # are never read (the match test takes label, y, x), so the script's name is bound to the same class
    # with those three set to None.
    from functools import partial
    rkp.KeypointDetection = partial(rdec.KeypointDetection, w=None, h=None, depth=None)
    return rnet, rcfg, rdec, rbox, rkp


class FakeBatch:
    """What the scripts read of a PoseSample. img carries the batch's index for the fake model."""

    def __init__(self, index, valid, label, center, size):
        B, N = valid.shape
        self.img = torch.full((B, 3, 2, 2), float(index))
        self.valid, self.label, self.center, self.size = valid, label, center, size
        self.depth = self.roll = self.pitch = self.yaw = torch.zeros((B, N))

    def to(self, device):
        return self


class FakeModel:
    def __init__(self, predictions):
        self.predictions = predictions

    def forward(self, img):
        return self.predictions[int(img[0, 0, 0, 0])]


def plant(rng, B, n_labels, N, n_invalid, logit_lo, logit_hi, centre_mode, exact_one=False):
    """One batch: truths, and maps with two peaks around every truth over a background of small distinct
    logits. Box mode: offsets in [0, R) and sizes around the truth's. Centre mode: the truths sit at planted
    distances from their peaks' cells."""
    valid = torch.ones((B, N), dtype=torch.bool)
    label = torch.from_numpy(rng.integers(0, n_labels, (B, N))).to(torch.int64)
    center = torch.from_numpy(0.2 + 0.6 * rng.random((B, N, 2))).float()
    size = torch.from_numpy(0.15 + 0.25 * rng.random((B, N, 2))).float()
    label[:, 1] = label[:, 0]  # truth 1: a shifted copy of truth 0, so records qualify for both
    center[:, 1] = center[:, 0] + 0.02
    size[:, 1] = size[:, 0]
    for b in range(B):
        valid[b, rng.choice(np.arange(2, N), size=n_invalid, replace=False)] = False
    heat = torch.from_numpy(-12.0 + 6.0 * rng.random((B, n_labels, H, W))).float()
    size_map = torch.from_numpy(0.05 + 0.3 * rng.random((B, H, W, 2))).float()
    offset = torch.from_numpy((1 << DOWNSAMPLES) * rng.random((B, H, W, 2))).float()
    for b in range(B):
        taken = []
        for m in range(N):
            cy, cx = int(center[b, m, 0] * H), int(center[b, m, 1] * W)
            for _ in range(2):
                for _ in range(100):
                    y, x = cy + int(rng.integers(-2, 3)), cx + int(rng.integers(-2, 3))
                    if 0 <= y < H and 0 <= x < W and all(max(abs(y - ty), abs(x - tx)) >= 2 for ty, tx in taken):
                        break
                else:
                    continue
                taken.append((y, x))
                lab = int(label[b, m]) if rng.random() < 0.85 else int((label[b, m] + 1) % n_labels)
                heat[b, lab, y, x] = float(logit_lo + (logit_hi - logit_lo) * rng.random())
                size_map[b, y, x] = size[b, m] * torch.from_numpy(0.6 + 0.8 * rng.random(2)).float()
        if exact_one:  # a sigmoid that is 1.0f: a score equal to the threshold 1
            y, x = taken[0]
            heat[b, int(label[b, 0]), y, x] = 30.0
    return valid, label, center, size, heat, size_map, offset


def make_case(refs, name, seed, n_batches, B, n_labels, N, n_invalid, centre_mode, match_threshold, thresholds):
    import eval_ref
    rnet, rcfg, rdec, rbox, rkp = refs
    mc = rcfg.ModelConfig([2] * 5, [16] * 6, H << DOWNSAMPLES, W << DOWNSAMPLES, DOWNSAMPLES, 1.0)
    no_angle = rcfg.AngleConfig(train=False, modulo=None)
    oc = rcfg.ObjectConfigSet([rcfg.ObjectConfig(id=f"o{i}", yaw=no_angle, pitch=no_angle, roll=no_angle,
                                                 train_depth=False, train_keypoints=centre_mode,
                                                 keypoints=[(0.0, 0.1, 0.1), (0.0, 0.1, -0.1), (0.0, -0.1, -0.1),
                                                            (0.0, -0.1, 0.1)] if centre_mode else [])
                               for i in range(n_labels)])
    thr32 = thresholds.numpy()
    while True:
        rng = np.random.default_rng(seed)
        planted = [plant(rng, B, n_labels, N, n_invalid, 2.0 if centre_mode else -3.0, 7.0 if centre_mode else 4.0,
                         centre_mode, exact_one=centre_mode) for _ in range(n_batches)]
        kp_heat = torch.from_numpy(-8.0 + 10.0 * rng.random((n_batches, B, oc.n_keypoints, H, W))).float() \
            if centre_mode else None
        kp_aff = torch.from_numpy(rng.standard_normal((n_batches, B, oc.n_keypoints, 2, H, W))).float() \
            if centre_mode else None
        preds, batches, recs, cnts = [], [], [], []
        ok = True
        for i, (valid, label, center, size, heat, size_map, offset) in enumerate(planted):
            preds.append(rnet.Prediction(heatmap=heat, keypoint_heatmap=kp_heat[i] if centre_mode else None,
                                         keypoint_affinity=kp_aff[i] if centre_mode else None, size=size_map,
                                         offset=offset, roll_bin=None, roll_offset=None, pitch_bin=None,
                                         pitch_offset=None, yaw_bin=None, yaw_offset=None, depth=None))
            batches.append(FakeBatch(i, valid, label, center, size))
            lowest = float(thresholds.min())
            if centre_mode:
                dets = rdec.decode_keypoints(preds[i], mc, oc, None, K, K, lowest, 0.5, 0.5)
            else:
                dets = rdec.decode(preds[i], mc, K, lowest)
            rec, cnt = eval_ref.records_from_detections(dets, K)
            recs.append(rec)
            cnts.append(cnt)
            peaks = rdec.heatmap_nms(torch.sigmoid(heat), 3).reshape(B, -1)
            top = torch.topk(peaks, K + 1).values.double()
            close = ((top[:, :-1] - top[:, 1:]) <= 2e-6 * top[:, :-1]) & (top[:, :-1] >= lowest)
            ok &= not bool(close.any())  # no tie among the records, or at the cut, for any decode to break
            d = np.abs(rec[..., 1].astype(np.float64)[..., None] - thr32.astype(np.float64))
            ok &= bool(((d > 1e-6) | (rec[..., 1][..., None] == thr32)).all())
            scene = eval_ref.scene_from_arrays(rec, cnt, valid.numpy(), label.numpy(), center.numpy(), size.numpy(),
                                               eval_ref.CENTRE if centre_mode else eval_ref.BOX, match_threshold)
            both = eval_ref.contention(scene)
            ok &= eval_ref.gap(scene) >= 1e-6 and not eval_ref.has_nan(scene) and both[0] >= 1 and both[1] >= 1
        if ok:
            break
        seed += 1000
        assert seed < 1000000, "no seed meets the fixture conditions"
    model = FakeModel(preds)
    pairs = []
    for t in thresholds:  # as the reference's evaluate_precision_recall_curve: a 0-d fp32 tensor per run
        if centre_mode:
            pairs.append(rkp.evaluate_precision_recall(model, mc, oc, None, batches, torch.device("cpu"), t, 0.5, 0.5,
                                                       match_threshold))
        else:
            pairs.append(rbox.evaluate_precision_recall(model, mc, batches, torch.device("cpu"), t, match_threshold))
    stack = lambda j: np.stack([p[j].numpy() for p in planted])
    arrays = dict(mode=1 if centre_mode else 0, match_threshold=float(match_threshold), seed=seed,
                  in_h=mc.in_h, in_w=mc.in_w, downsamples=DOWNSAMPLES, n_labels=n_labels, n_detections=K,
                  valid=stack(0), label=stack(1), center=stack(2), size=stack(3), heatmap=stack(4), size_map=stack(5),
                  offset=stack(6), records=np.stack(recs), counts=np.stack(cnts), score_thresholds=thr32,
                  precision=np.array([float(p) for p, _ in pairs], dtype=np.float64),
                  recall=np.array([float(r) for _, r in pairs], dtype=np.float64))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
    print(name, "seed", seed, "counts", np.stack(cnts).tolist())
    for t, (p, r) in zip(thr32, pairs):
        print(f"  t = {t:.4f}: precision {float(p):.4f} recall {float(r):.4f}")


def main():
    refs = _import_reference()
    box_thr = torch.linspace(0, 1, 10)  # evaluate.py:213
    only = sys.argv[1:]
    if only and only[0] == "centre":  # (the box fixtures take longer to draw)
        make_case(refs, "eval_centre_b2_l1_24x32", 23, 2, 2, 1, 5, 1, True, 0.07, torch.linspace(0.9, 1, 10))
        return
    make_case(refs, "eval_box_b3_l3_24x32", 21, 2, 3, 3, 6, 1, False, 0.3, box_thr)
    make_case(refs, "eval_box_iou0_b3_l3_24x32", 22, 2, 3, 3, 6, 1, False, 0.0, box_thr)
    make_case(refs, "eval_centre_b2_l1_24x32", 23, 2, 2, 1, 5, 1, True, 0.07, torch.linspace(0.9, 1, 10))


if __name__ == "__main__":
    main()
