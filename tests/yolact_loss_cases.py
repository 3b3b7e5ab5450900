"""Cases of the YOLACT training loss (tauv_vision_amd.yolact_loss, csrc/yolact_loss.hip): the case
dictionaries and the seeded `make_inputs(case)`. torch and numpy only; the same recipe makes the inputs of
the reference run that tests/golden/gen_golden_yolact_loss.py stores.

Every case's inputs keep clear of the places where the reference itself is not well defined
(`input_conditions`, checked on the float64 restatement by test_yolact_loss_ref_cpu.py):
  * |match_iou - threshold| >= 1e-4 for both thresholds;
  * where the best IoU is positive, the second best at that anchor is at least 1e-5 lower;
  * per sample 1 <= k <= n_negative - 1, and the k-th and (k+1)-th smallest background probabilities among
    the negatives differ by at least 1e-4 relative (case D has no positive by construction: k = 0 there);
  * no mask logit of a positive within 0.05 of +-ln 9999;
  * no smooth-L1 argument within 1e-4 of +-1 or of 0;
  * truth boxes of positive height and width;
  * no box_to_mask edge within 1e-3 of an integer pixel coordinate.
`find_seed(case)` re-draws with the next seed until they hold; the seed found is recorded in the case.
"""
from math import log, sqrt
from types import SimpleNamespace

import numpy as np
import torch

PREDICTION = ("classification", "box_encoding", "mask_coeff", "anchor", "mask_prototype")
TRUTH = ("truth_valid", "truth_classification", "truth_box", "truth_seg_map", "truth_img_valid")
BACKGROUND = 255  # the seg map's value outside every object: no truth index

_A = dict(B=2, in_h=64, in_w=96, levels=((8, 12), (4, 6), (2, 3)), scales=(12, 24, 48), C=5, P=8, h=16, w=24, T=4,
          invalid=((0, 3), (1, 1)), stripe=(40, 52), unpainted=(), ratio=3, seed=1)
CASES = {
    # A: tiny. 378 anchors, one invalid truth per sample, a stripe of truth_img_valid false
    "yolact_loss_a": dict(_A),
    # B: past one workgroup, off every alignment: 1122 anchors, 23 x 37 prototypes from a 90 x 150 input
    "yolact_loss_b": dict(B=2, in_h=90, in_w=150, levels=((13, 21), (7, 11), (4, 6)), scales=(14, 28, 56), C=3, P=32,
                          h=23, w=37, T=5, invalid=(), stripe=(100, 117), unpainted=(), ratio=3, seed=4),
    # C: odd P, one sample, one truth
    "yolact_loss_c": dict(_A, B=1, P=5, T=1, invalid=(), seed=2),
    # D: no positive: every truth invalid
    "yolact_loss_d": dict(_A, invalid="all"),
    # E: a valid truth whose index does not occur in the seg map
    "yolact_loss_e": dict(_A, unpainted=((0, 1), (1, 2)), seed=1),
}
ASPECT_RATIOS = (1.0, 0.5, 2.0)


def config_of(c, **over):
    """The fields of the reference's ModelConfig that the loss and get_anchor read."""
    f = dict(in_h=c["in_h"], in_w=c["in_w"], anchor_scales=c["scales"], anchor_aspect_ratios=ASPECT_RATIOS,
             box_variances=(0.1, 0.2), iou_pos_threshold=0.5, iou_neg_threshold=0.4,
             negative_example_ratio=c["ratio"], n_classes=c["C"], n_prototype_masks=c["P"])
    f.update(over)
    return SimpleNamespace(**f)


def get_anchor(fpn_i, fpn_size, config):
    """anchors.py:9-41: (y, x, h, w) anchors of one pyramid level, [1, n, 4], one block per aspect ratio."""
    n = len(config.anchor_aspect_ratios)
    y = (torch.arange(0, fpn_size[0]) + 0.5) / fpn_size[0]
    x = (torch.arange(0, fpn_size[1]) + 0.5) / fpn_size[1]
    y, x = torch.meshgrid(y, x, indexing="ij")
    y, x = torch.tile(y.flatten(), (1, n)), torch.tile(x.flatten(), (1, n))
    in_size = (config.in_h + config.in_w) / 2
    scale = config.anchor_scales[fpn_i]
    cells = fpn_size[0] * fpn_size[1]
    hs = torch.cat([torch.full((1, cells), (scale / in_size) * sqrt(r)) for r in config.anchor_aspect_ratios], dim=-1)
    ws = torch.cat([torch.full((1, cells), (scale / in_size) / sqrt(r)) for r in config.anchor_aspect_ratios], dim=-1)
    return torch.stack((y, x, hs, ws), dim=1).permute(0, 2, 1)


def make_inputs(c, seed=None):
    """-> dict of the ten tensors of PREDICTION + TRUTH (CPU; fp32, int64 classes, uint8 seg map, bool)."""
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    cfg = config_of(c)
    B, T, C, P, h, w, in_h, in_w = c["B"], c["T"], c["C"], c["P"], c["h"], c["w"], c["in_h"], c["in_w"]
    anchor = torch.cat([get_anchor(i, s, cfg) for i, s in enumerate(c["levels"])], dim=1).contiguous()
    A = anchor.shape[1]
    # truth boxes: jittered anchors, so that each has a few anchors past the positive threshold
    pick = torch.randint(0, A, (B, T), generator=g)
    base = anchor[0][pick]
    jitter = (torch.rand((B, T, 2), generator=g) - 0.5) * 0.3
    grow = torch.exp((torch.rand((B, T, 2), generator=g) - 0.5) * 0.3)
    truth_box = torch.cat((base[..., :2] + jitter * base[..., 2:], base[..., 2:] * grow), dim=-1).contiguous()
    truth_valid = torch.ones((B, T), dtype=torch.bool)
    if c["invalid"] == "all":
        truth_valid[:] = False
    else:
        for b, t in c["invalid"]:
            truth_valid[b, t] = False
    truth_classification = torch.randint(1, C, (B, T), generator=g)
    # the seg map holds the truth's index inside an ellipse in its box; later truths paint over earlier ones
    seg = torch.full((B, in_h, in_w), BACKGROUND, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(in_h) + 0.5, torch.arange(in_w) + 0.5, indexing="ij")
    for b in range(B):
        for t in range(T):
            if (b, t) in c["unpainted"]:
                continue
            cy, cx, bh, bw = (float(v) for v in truth_box[b, t] * torch.tensor([in_h, in_w, in_h, in_w]))
            inside = ((yy - cy) / (bh / 2)) ** 2 + ((xx - cx) / (bw / 2)) ** 2 <= 1.0
            seg[b][inside] = t
    truth_img_valid = torch.ones((B, in_h, in_w), dtype=torch.bool)
    truth_img_valid[:, :, c["stripe"][0]:c["stripe"][1]] = False
    classification = 2.0 * torch.randn((B, A, C), generator=g)
    box_encoding = 1.5 * torch.randn((B, A, 4), generator=g)
    mask_coeff = torch.tanh(torch.randn((B, A, P), generator=g))
    # most logits stay well inside the clamp bounds (+-ln 9999 = +-9.21); one pixel in a hundred is scaled far
    # past them, on either side, so that few logits come near a bound
    spike = 1.0 + 24.0 * (torch.rand((B, 1, h, w), generator=g) < 0.01).float()
    mask_prototype = (3.3 / sqrt(P)) * spike * torch.relu(torch.randn((B, P, h, w), generator=g))
    return dict(classification=classification, box_encoding=box_encoding, mask_coeff=mask_coeff, anchor=anchor,
                mask_prototype=mask_prototype, truth_valid=truth_valid, truth_classification=truth_classification,
                truth_box=truth_box, truth_seg_map=seg, truth_img_valid=truth_img_valid)


def input_conditions(c, inputs, state):
    """The conditions of the module docstring on one case, as a list of the names of those that fail.
    `state` is the float64 restatement's record (yolact_loss_ref.loss_ref)."""
    cfg = config_of(c)
    bad = []
    iou = state["match_iou"]
    for name, th in (("pos", cfg.iou_pos_threshold), ("neg", cfg.iou_neg_threshold)):
        if float((iou - th).abs().min()) < 1e-4:
            bad.append("iou within 1e-4 of the %s threshold" % name)
    if state["iou"].shape[2] > 1:
        top = torch.topk(state["iou"], 2, dim=2).values
        close = (top[..., 0] > 0) & (top[..., 0] - top[..., 1] < 1e-5)
        if bool(close.any()):
            bad.append("second best iou within 1e-5 of the best")
    if not bool((inputs["truth_box"][..., 2:] > 0).all()):
        bad.append("truth box without height or width")
    none_expected = c["invalid"] == "all"
    for b in range(c["B"]):
        pos, neg = state["positive"][b], state["negative"][b]
        k, n_neg = cfg.negative_example_ratio * int(pos.sum()), int(neg.sum())
        if none_expected:
            if k != 0:
                bad.append("a positive in the case without one")
            continue
        if not 1 <= k <= n_neg - 1:
            bad.append("k = %d of %d negatives in sample %d" % (k, n_neg, b))
            continue
        p = torch.sort(state["background"][b][neg]).values
        if float(p[k] - p[k - 1]) < 1e-4 * float(p[k]):
            bad.append("k-th and (k+1)-th background probabilities within 1e-4 relative in sample %d" % b)
    ln = log(9999.0)
    if state["mask_logits"].numel() and float((state["mask_logits"].abs() - ln).abs().min()) < 0.05:
        bad.append("a mask logit within 0.05 of +-ln 9999")
    d = state["box_args"]
    if d.numel() and (float((d.abs() - 1).abs().min()) < 1e-4 or float(d.abs().min()) < 1e-4):
        bad.append("a smooth-L1 argument within 1e-4 of +-1 or 0")
    e = state["box_edges"]
    if e.numel() and float((e - torch.round(e)).abs().min()) < 1e-3:
        bad.append("a box_to_mask edge within 1e-3 of a pixel coordinate")
    return bad


def saturates(state):
    """Whether the positives' mask logits pass both clamp bounds somewhere."""
    z, ln = state["mask_logits"], log(9999.0)
    return bool(z.numel() and float(z.max()) > ln and float(z.min()) < -ln)


def find_seed(c, first=1, tries=200):
    """The first seed from `first` on whose draw meets the conditions (and saturates both clamp bounds
    where the case has positives)."""
    import yolact_loss_ref as R
    for seed in range(first, first + tries):
        inputs = make_inputs(c, seed)
        state = R.loss_ref(R.prediction_of(inputs, torch.float64), R.truth_of(inputs), config_of(c))[2]
        if not input_conditions(c, inputs, state) and (c["invalid"] == "all" or saturates(state)):
            return seed
    raise RuntimeError("no seed meets the input conditions")


def stored(inputs):
    """The inputs as the numpy arrays a fixture stores (in_ prefix)."""
    return {"in_" + k: v.numpy().copy() for k, v in inputs.items()}


def loaded(npz):
    """The inputs of a fixture as torch tensors."""
    return {k: torch.from_numpy(np.array(npz["in_" + k])) for k in PREDICTION + TRUTH}
