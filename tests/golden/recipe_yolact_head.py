"""Cases and seeded inputs of the YOLACT neck + head goldens (tests/golden/gen_golden_yolact_head.py):
FeaturePyramid (feature_pyramid.py:8-58), PredictionHead (prediction_head.py:9-143), Masknet and the
concatenation of Yolact.forward (model.py:31-60), everything after the backbone.

The smallest shapes at which each piece can still go wrong:
  A  five levels 9x11, 5x6, 3x3, 2x2, 1x1 (143 anchors): non-integer, per-axis-different bilinear
     ratios, a 1x1 level, 20 stacked head columns
  B  branch blocks (the three final convs cannot be stacked), three aspect ratios (the
     ratio-innermost row order against get_anchor's ratio-major blocks), 969 anchors
  C  exact x2 ratios, no trunk block, no extra levels (three levels only), 24 stacked columns
  D  the benchmark geometry (550 x 550: 69 / 35 / 18 maps of a ResNet's 128 / 256 / 512 channels,
     F = 256): inputs regenerated from the seed, head outputs stored in full, prototypes as a seeded
     sample + per-channel sums
`layers` = (n_prediction_head_layers, n_classification_layers, n_box_layers, n_mask_layers).
"""
import json
import os

import torch

from recipe import seeded_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES, VAR = (24, 48, 96, 192, 384), (0.1, 0.2)
HEAD_CASES = [
    dict(name="yolact_head_a", depths=(16, 32, 64), F=32, C=7, k=8, ars=(1,), layers=(1, 0, 0, 0), down=2, batch=2,
         sizes=((9, 11), (5, 6), (3, 3)), in_h=72, in_w=88, seed=400, full=True),
    dict(name="yolact_head_b", depths=(16, 32, 64), F=64, C=3, k=32, ars=(1 / 2, 1, 2), layers=(1, 1, 0, 1), down=2,
         batch=1, sizes=((12, 20), (6, 10), (3, 5)), in_h=96, in_w=160, seed=410, full=True),
    dict(name="yolact_head_c", depths=(16, 32, 64), F=32, C=2, k=5, ars=(1, 2), layers=(0, 0, 0, 0), down=0, batch=1,
         sizes=((8, 8), (4, 4), (2, 2)), in_h=64, in_w=64, seed=420, full=True),
    dict(name="yolact_head_d", depths=(128, 256, 512), F=256, C=7, k=8, ars=(1,), layers=(1, 0, 0, 0), down=2, batch=1,
         sizes=((69, 69), (35, 35), (18, 18)), in_h=550, in_w=550, seed=430, full=False),
]
# The end-to-end case: case A's network on one frame, through box_decode -> nms(100, 0.5, 0.05) ->
# assemble_mask. Conditioned so that the comparison of NMS indices is exact, not "mostly": `bg_bias`
# is added to the background logit's bias of the classification layer (a trained detector calls most
# anchors background; seeded weights call none), so only a handful of anchors pass the confidence
# threshold, and the generator tries seeds from `seed` on until every decision nms takes has a margin
# of 1e-3 (E2E_MARGIN); the seed it found is stored in the fixture.
E2E_CASE = dict(HEAD_CASES[0], name="yolact_head_e2e", batch=1, seed=500, bg_bias=6.0)
E2E_NMS = (100, 0.5, 0.05)
E2E_MARGIN = 1e-3
HEAD_SAMPLES = 4096
_LAYOUTS = None


def head_case(name):
    for c in HEAD_CASES + [E2E_CASE]:
        if c["name"] == name:
            return c
    raise KeyError(name)


def head_layout(case):
    """[(key, shape)] of the reference modules' state_dict — `_feature_pyramid.*`, `_masknet.*`,
    `_prediction_head.*` in Yolact's registration order — as the generator recorded it."""
    global _LAYOUTS
    if _LAYOUTS is None:
        with open(os.path.join(HERE, "yolact_head_layouts.json")) as f:
            _LAYOUTS = json.load(f)
    return [(k, tuple(s)) for k, s in _LAYOUTS[case["name"]]]


def head_level_sizes(case):
    out = [tuple(s) for s in case["sizes"]]
    for _ in range(case["down"]):
        out.append(((out[-1][0] - 1) // 2 + 1, (out[-1][1] - 1) // 2 + 1))
    return out


def head_inputs(case, layout=None):
    """(state_dict, backbone maps [B, depth_i, h_i, w_i]) of a case."""
    sd = seeded_state_dict(layout if layout is not None else head_layout(case), conv_seed=case["seed"],
                           aux_seed=case["seed"] + 1)
    if case.get("bg_bias"):  # channel a * (C + 1) is aspect ratio a's background logit
        sd["_prediction_head._classification_layer.bias"][::case["C"] + 1] += case["bg_bias"]
    g = torch.Generator().manual_seed(case["seed"] + 2)
    maps = [torch.randn((case["batch"], c, h, w), generator=g) for c, (h, w) in zip(case["depths"], case["sizes"])]
    return sd, maps


def nms_margins(cls, box, top_k, iou_threshold, confidence_threshold, iou_matrix):
    """(confidence margin, IoU margin, n) of nms (nms.py:7-29) on batch 0, n = the candidates at or
    above the confidence threshold. Its result is decided by their order (the smallest gap between
    consecutive sorted confidences), by which anchors they are (every anchor's distance to the
    threshold) and by the pairwise IoUs among them against the IoU threshold: an error below both
    margins cannot change the indices it returns. Needs n < top_k (no cut at the top-k rank)."""
    conf = torch.softmax(cls[0], dim=-1)[:, 1:].max(dim=-1).values
    conf, order = conf.sort(descending=True)
    n = int((conf >= confidence_threshold).sum())
    assert n < top_k, f"{n} candidates reach the top-k cut"
    gaps = torch.cat([conf[:n - 1] - conf[1:n], (conf - confidence_threshold).abs()]) if n else conf.new_ones(1)
    b = box[0, order[:n]].unsqueeze(0)
    iou = iou_matrix(b, b)[0]
    pairs = iou[torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)]
    iou_margin = float((pairs - iou_threshold).abs().min()) if pairs.numel() else float("inf")
    return float(gaps.min()), iou_margin, n


def head_sample_index(case):
    """Seeded flat positions into the prototypes [B, k, 4h, 4w] of the sampled (full=False) cases."""
    h, w = case["sizes"][0]
    g = torch.Generator().manual_seed(case["seed"] + 3)
    return torch.randint(0, case["batch"] * case["k"] * 16 * h * w, (HEAD_SAMPLES,), generator=g)
