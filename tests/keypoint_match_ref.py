"""Test infrastructure of the keypoint matching (tv_match_keypoints, csrc/keypoints.hip): planted
scenes, the oracle's own assignment as arrays, and a checker that REPLAYS a matching instead of
comparing it for equality.

Why a replay. The matching is greedy: keypoint k goes to the candidate of the smallest
|atan2(ay, ax) - atan2(ky - y, kx - x)|. Grid cells are often collinear, so two candidates can have
exactly or nearly the same error, and the device's double atan2 is not bit-identical to libm's: on
such a step either choice is right, and every later step depends on it. The checker therefore walks
the keypoints in rank order, keeps the slot state implied by the matching's OWN kp_det, and at each
step recomputes the candidates and the double errors on the CPU. It requires
  * -1 exactly when there is no candidate, or the rank is at or past the count;
  * otherwise a choice that is a candidate;
  * the first-index argmin (errs.index(min(errs)), the first candidate when every error is NaN)
    whenever the runner-up is more than TIE away; inside TIE any candidate within TIE of the minimum;
  * slot_kp and n_matched the exact inverse of kp_det.
TIE = 1e-9: errors of distinct directions on these grids differ by >= 2e-9 where they differ at all,
the device atan2 by about 1e-15. A step whose runner-up is inside TIE is a "tied" step; the tests cap
them at 5 % of the steps with two or more candidates, so the check cannot pass by ties alone.

Scenes are planted, not random heatmaps: background logit -8, n_obj object peaks and n_kp keypoint
peaks at cells drawn by randperm(H * W), each in a random channel, distinct logits (linspace(-1, 3)
for objects, linspace(-2, 3) for keypoints, shuffled), affinity randn, thresholds 0.5 / 0.3."""
from math import atan2
from types import SimpleNamespace

import numpy as np
import torch

import oracle

TIE = 1e-9
TIE_CAP = 0.05

# name -> B, H, W, keypoint slots per label, planted objects, planted keypoints, K, K_kp
SCENES = {
    "A": dict(B=3, H=24, W=40, slots=[3, 0, 8, 1], n_obj=12, n_kp=70, K=10, K_kp=50),
    "B": dict(B=2, H=40, W=64, slots=[2, 32], n_obj=80, n_kp=200, K=70, K_kp=130),
    "C": dict(B=1, H=30, W=40, slots=[1, 1, 1, 1], n_obj=12, n_kp=70, K=10, K_kp=50),
    # B with few objects: in B itself about 30 objects share a label and at most a dozen keypoints ask for
    # one slot, so no keypoint is ever left without a candidate there; here most are
    "D": dict(B=2, H=40, W=64, slots=[2, 32], n_obj=6, n_kp=200, K=70, K_kp=130),
}
THR, KP_THR = 0.5, 0.3


def _plant(g, B, C, H, W, n, lo, hi):
    heat = torch.full((B, C, H, W), -8.0)
    for b in range(B):
        cells = torch.randperm(H * W, generator=g)[:n]
        ch = torch.randint(0, C, (n,), generator=g)
        logit = torch.linspace(lo, hi, n)[torch.randperm(n, generator=g)]
        heat[b, ch, cells // W, cells % W] = logit
    return heat


def make_scene(name, seed, **override):
    """SimpleNamespace(pred (CPU tensors in the reference's Prediction layout), owner [(label, slot)] per
    flat keypoint index, slots, max_slots, B, H, W, K, K_kp, thr, kp_thr)."""
    p = dict(SCENES[name], **override)
    B, H, W, slots = p["B"], p["H"], p["W"], p["slots"]
    g = torch.Generator().manual_seed(seed)
    C, C_kp = len(slots), sum(slots)
    heat = _plant(g, B, C, H, W, p["n_obj"], -1.0, 3.0)
    kheat = _plant(g, B, C_kp, H, W, p["n_kp"], -2.0, 3.0)
    pred = SimpleNamespace(heatmap=heat, keypoint_heatmap=kheat,
                           keypoint_affinity=torch.randn((B, C_kp, 2, H, W), generator=g),
                           size=torch.rand((B, H, W, 2), generator=g), offset=torch.zeros((B, H, W, 2)),
                           depth=torch.randn((B, H, W, 1), generator=g))
    owner = [(lab, s) for lab, n in enumerate(slots) for s in range(n)]
    return SimpleNamespace(pred=pred, owner=owner, slots=list(slots), max_slots=max(slots), B=B, H=H, W=W, K=p["K"],
                           K_kp=p["K_kp"], thr=THR, kp_thr=KP_THR)


def object_config(scene):
    """The tauv_vision_amd ObjectConfigSet of a scene (one object per label, `slots[label]` keypoints)."""
    import tauv_vision_amd as tv
    A = tv.AngleConfig
    return tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), True, n > 0,
                                               [(0.1 * s, 0.0, 0.0) for s in range(n)] if n else None)
                               for i, n in enumerate(scene.slots)])


def oracle_records(scene):
    """The record arrays tv_decode (mode 1) writes, from the oracle's own functions: obj [B, K, 10] fp32,
    obj_n [B], kp [B, K_kp, 10], kp_n [B] (label, score, y, x, h, w, depth, flat index, affinity y, x)."""
    pr, H, W = scene.pred, scene.H, scene.W
    depth = 1 / torch.sigmoid(pr.depth)

    def records(heat, K, thr, keypoints):
        index, label, score = oracle.heatmap_detect(oracle.heatmap_nms(torch.sigmoid(heat), 3), K)
        rec = np.zeros((scene.B, K, 10), dtype=np.float32)
        n = np.zeros((scene.B,), dtype=np.int32)
        for b in range(scene.B):
            for k in range(K):
                if score[b, k] < thr:
                    break
                iy, ix, lab = index[b, k, 0], index[b, k, 1], int(label[b, k])
                aff = pr.keypoint_affinity[b, lab, :, iy, ix] if keypoints else (0.0, 0.0)
                rec[b, k] = (lab, float(score[b, k]), float(iy / H), float(ix / W), float(pr.size[b, iy, ix, 0]),
                             float(pr.size[b, iy, ix, 1]), 0.0 if keypoints else float(depth[b, iy, ix]),
                             (lab * H + int(iy)) * W + int(ix), float(aff[0]), float(aff[1]))
                n[b] = k + 1
        return rec, n

    obj, obj_n = records(pr.heatmap, scene.K, scene.thr, False)
    kp, kp_n = records(pr.keypoint_heatmap, scene.K_kp, scene.kp_thr, True)
    return obj, obj_n, kp, kp_n


def assignment_arrays(kp_det, K, max_slots, owner, kp):
    """(slot_kp [B, K, max_slots], n_matched [B, K]): the inverse of kp_det [B, K_kp]."""
    B, K_kp = kp_det.shape
    slot_kp = np.full((B, K, max_slots), -1, dtype=np.int32)
    n_matched = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        for k in range(K_kp):
            d = int(kp_det[b, k])
            if d >= 0:
                slot_kp[b, d, owner[int(kp[b, k, 0])][1]] = k
                n_matched[b, d] += 1
    return slot_kp, n_matched


def oracle_assignment(scene, records=None):
    """(kp_det, slot_kp, n_matched) of oracle.decode_keypoints' own matching: its per-detection keypoint
    lists mapped back to keypoint ranks through (score, y, x), which identify a keypoint record."""
    obj, obj_n, kp, kp_n = records or oracle_records(scene)
    dets = oracle.decode_keypoints(scene.pred, scene.H, scene.W, scene.owner, scene.K, scene.K_kp, scene.thr,
                                   scene.kp_thr)
    kp_det = np.full((scene.B, scene.K_kp), -1, dtype=np.int32)
    for b, image in enumerate(dets):
        assert len(image) == obj_n[b]
        rank = {(float(r[1]), float(r[2]), float(r[3])): k for k, r in enumerate(kp[b, :kp_n[b]])}
        assert len(rank) == kp_n[b]
        for d, det in enumerate(image):
            for point, score in zip(det["keypoints"], det["keypoint_scores"]):
                if point is not None:
                    kp_det[b, rank[(score, point[0], point[1])]] = d
    return (kp_det,) + assignment_arrays(kp_det, scene.K, scene.max_slots, scene.owner, kp)


def check_matching(obj, obj_n, kp, kp_n, owner, max_slots, kp_det, slot_kp, n_matched, tie=TIE):
    """Replay a matching (see the module text). Raises AssertionError at the first violation; returns the
    event counts: steps (keypoints below the count), multi (steps with >= 2 candidates), none (steps
    without a candidate), excluded (steps where an object of the owner label was left out because its
    slot was taken), tied (multi steps whose runner-up is within `tie` of the minimum), nan (steps whose
    errors are all NaN)."""
    obj, kp, kp_det, slot_kp, n_matched = (np.asarray(a) for a in (obj, kp, kp_det, slot_kp, n_matched))
    B, K = obj.shape[:2]
    K_kp = kp.shape[1]
    assert kp_det.shape == (B, K_kp) and slot_kp.shape == (B, K, max_slots) and n_matched.shape == (B, K)
    stats = dict(steps=0, multi=0, none=0, excluded=0, tied=0, nan=0)
    for b in range(B):
        taken = [[False] * max_slots for _ in range(K)]
        for k in range(K_kp):
            c = int(kp_det[b, k])
            where = f"image {b}, keypoint {k}"
            if k >= kp_n[b]:
                assert c == -1, f"{where}: at or past the count {kp_n[b]} but matched to {c}"
                continue
            stats["steps"] += 1
            label, slot = owner[int(kp[b, k, 0])]
            same = [d for d in range(int(obj_n[b])) if int(obj[b, d, 0]) == label]
            cands = [d for d in same if not taken[d][slot]]
            stats["excluded"] += len(cands) < len(same)
            if not cands:
                stats["none"] += 1
                assert c == -1, f"{where}: no candidate but matched to {c}"
                continue
            assert c in cands, f"{where}: matched to {c}, the candidates are {cands}"
            ky, kx, ay, ax = (float(kp[b, k, j]) for j in (2, 3, 8, 9))
            ang = atan2(ay, ax)
            errs = [abs(ang - atan2(ky - float(obj[b, d, 2]), kx - float(obj[b, d, 3]))) for d in cands]
            if len(cands) >= 2:
                stats["multi"] += 1
            if all(e != e for e in errs):
                stats["nan"] += 1
                assert c == cands[0], f"{where}: NaN errors go to the first candidate {cands[0]}, not {c}"
            else:
                best = errs.index(min(errs))
                order = sorted(errs)
                if len(errs) >= 2 and order[1] - order[0] <= tie:
                    stats["tied"] += 1
                    assert errs[cands.index(c)] - order[0] <= tie, \
                        f"{where}: {c} (error {errs[cands.index(c)]!r}) is not among the tied minima ({order[0]!r})"
                else:
                    assert c == cands[best], f"{where}: matched to {c} (error {errs[cands.index(c)]!r}), the " \
                                             f"minimum is at {cands[best]} ({errs[best]!r})"
            taken[c][slot] = True
    want_slot, want_n = assignment_arrays(kp_det, K, max_slots, owner, kp)
    assert np.array_equal(slot_kp, want_slot), "slot_kp is not the inverse of kp_det"
    assert np.array_equal(n_matched, want_n), "n_matched is not the inverse of kp_det"
    return stats


def multi_step(scene, rec, kp_det):
    """(b, k, chosen d, another candidate d2 with a clearly larger error) of one step with >= 2 candidates."""
    obj, obj_n, kp, kp_n = rec
    for b in range(scene.B):
        taken = set()
        for k in range(int(kp_n[b])):
            label, slot = scene.owner[int(kp[b, k, 0])]
            cands = [d for d in range(int(obj_n[b])) if int(obj[b, d, 0]) == label and (d, slot) not in taken]
            c = int(kp_det[b, k])
            if c >= 0:
                taken.add((c, slot))
            if len(cands) >= 2:
                ang = atan2(float(kp[b, k, 8]), float(kp[b, k, 9]))
                err = {d: abs(ang - atan2(float(kp[b, k, 2]) - float(obj[b, d, 2]),
                                          float(kp[b, k, 3]) - float(obj[b, d, 3]))) for d in cands}
                worse = [d for d in cands if err[d] > err[c] + 1e-3]
                if worse:
                    return b, k, c, worse[0]
    raise AssertionError("no step with two clearly different candidates")


def assert_tie_cap(stats, what=""):
    assert stats["tied"] <= TIE_CAP * stats["multi"], f"{what}: {stats['tied']} tied of {stats['multi']} steps with " \
                                                     f">= 2 candidates (cap {TIE_CAP:.0%})"
