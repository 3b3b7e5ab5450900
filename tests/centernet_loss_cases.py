"""The input recipe of the CenterNet loss tests: seeded truth batches and synthetic predictions in the
reference model's layout. It imports torch and numpy only. tests/golden/gen_golden_loss.py made the stored
fixtures (tests/golden/loss_*.npz) from CASES with it (test_centernet_loss_ref_cpu.py checks that
make_case(CASES[name]) still reproduces every stored input bit for bit), and the generated cases
(GENERATED) reach the launcher's schedules the fixtures' maps are too small for; they are checked against
the float64 restatement (centernet_loss_ref.py) alone.

Conditions on the inputs (not tolerances), asserted for every case by the CPU suite:
  * no heatmap / keypoint-heatmap logit z, as fp32, fp16 or bf16, has | |z| - ln 9999 | < 0.05: there
    sigmoid or 1 - sigmoid sits at focal_loss's 1e-4 clamp, whose gradient is discontinuous, so fp32
    and float64 legitimately disagree by O(1) on such an element;
  * no normalised truth angle lies within 0.01 rad of a bin edge (bin membership is a step);
  * no center * in / ratio or keypoint_center * in / ratio lies within 1e-4 of an integer (the cell index
    truncates: the fp32 and the float64 cell could differ).
"""
from math import log, pi
from types import SimpleNamespace

import numpy as np
import torch

HEADS = ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size", "offset", "roll_bin", "roll_offset", "pitch_bin",
         "pitch_offset", "yaw_bin", "yaw_offset", "depth")
TRUTH = ("valid", "label", "center", "size", "roll", "pitch", "yaw", "depth", "keypoint_valid", "keypoint_label",
         "keypoint_center", "keypoint_object_index")
CLAMP_Z = log(9999.0)
LOGIT_BAND, ANGLE_BAND, CELL_BAND = 0.05, 0.01, 1e-4

# name: B, in_h, in_w, downsamples, keypoints per label, n_objects, n_instances, (roll, pitch, yaw) modulo or
# None (no angle heads), depth head, focal (alpha, beta), sigmas, lambdas (kp heatmap, affinity, size, offset,
# angle, depth), bin overlap, seed
CASES = {
    "loss_allheads_b2_24x40": dict(B=2, in_h=96, in_w=160, ds=2, kps=[2, 1], n_obj=5, n_inst=7,
                                   moduli=(pi / 2, pi, 2 * pi), depth=True, focal=(2.0, 4.0), sigmas=(2.0, 3.0),
                                   lambdas=(0.7, 0.3, 0.9, 1.3, 0.45, 0.15), overlap=pi / 3, seed=21),
    "loss_torpedo_b3_23x40": dict(B=3, in_h=92, in_w=160, ds=2, kps=[1, 1, 1, 1], n_obj=4, n_inst=6, moduli=None,
                                  depth=False, focal=(1.5, 3.0), sigmas=(1.5, 2.5),
                                  lambdas=(1.1, 0.2, 0.8, 1.2, 1.0, 1.0), overlap=pi / 3, seed=22),
    "loss_tiny_b1_5x7": dict(B=1, in_h=5, in_w=7, ds=0, kps=[0], n_obj=3, n_inst=2, moduli=None, depth=False,
                             focal=(2.0, 4.0), sigmas=(1.0, 1.5), lambdas=(1.0, 1.0, 0.6, 1.4, 1.0, 1.0), overlap=pi / 3,
                             seed=23),
}

# The schedules of loss.hip's launcher no stored fixture reaches (a dense workgroup is 256 threads of 4
# cells on the vector route, of 1 cell on the scalar route; gx workgroups per plane):
#   rows   18x30: vector route (540 cells, 135 live threads, gx 1; scalar would be 3), W % 4 = 2: a thread's
#          four cells straddle two rows
#   vec3   36x62: vector route, gx 3, the last workgroup 46 threads live (scalar 9), W % 4 = 2; `crowd`
#          adds a cell of four objects whose first is invalid and two off-frame objects in one corner cell
#   scal3  17x31: 527 cells, scalar route, gx 3, the last workgroup 15 live; powf for alpha, beta, alpha - 1
#   many   4x6, B 260: the object kernel's 5 workgroups of 64 with a tail of 4; finalize's strided loops
#          over 260 samples and 1040 dense partials
GENERATED = {
    "rows": dict(B=2, in_h=72, in_w=120, ds=2, kps=[2, 1], n_obj=5, n_inst=7, moduli=(pi / 2, pi, 2 * pi),
                 depth=True, focal=(2.0, 4.0), sigmas=(2.0, 3.0), lambdas=(0.7, 0.3, 0.9, 1.3, 0.45, 0.15),
                 overlap=pi / 3, seed=31),
    "vec3": dict(B=2, in_h=144, in_w=248, ds=2, kps=[2, 1], n_obj=12, n_inst=9, moduli=(pi / 2, pi, 2 * pi),
                 depth=True, focal=(3.0, 2.0), sigmas=(2.5, 3.5), lambdas=(0.6, 0.4, 0.9, 1.3, 0.45, 0.15),
                 overlap=pi / 3, seed=32, crowd=True),
    "scal3": dict(B=3, in_h=34, in_w=62, ds=1, kps=[1, 2], n_obj=4, n_inst=5, moduli=None, depth=False,
                  focal=(2.5, 3.5), sigmas=(1.5, 2.5), lambdas=(1.1, 0.2, 0.8, 1.2, 1.0, 1.0), overlap=pi / 3,
                  seed=33),
    "many": dict(B=260, in_h=16, in_w=24, ds=2, kps=[1, 1], n_obj=3, n_inst=2, moduli=(pi / 2, pi, 2 * pi),
                 depth=True, focal=(2.0, 4.0), sigmas=(1.0, 1.5), lambdas=(0.7, 0.3, 0.9, 1.3, 0.45, 0.15),
                 overlap=pi / 3, seed=34),
}


def spec_of(name):
    return CASES[name] if name in CASES else GENERATED[name]


def out_of_band(z):
    bad = torch.zeros_like(z, dtype=torch.bool)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        bad |= (z.to(dt).float().abs() - CLAMP_Z).abs() < LOGIT_BAND
    return torch.where(bad, torch.sign(z) * (CLAMP_Z + 0.25), z)


def make_truth(c, H, W, g):
    """-> a namespace of the TRUTH tensors (the reference's PoseSample fields the loss reads)."""
    B, n_obj, n_inst, L, K = c["B"], c["n_obj"], c["n_inst"], len(c["kps"]), sum(c["kps"])
    valid = torch.rand((B, n_obj), generator=g) < 0.75
    valid[0, 0] = valid[0, 1] = True
    valid[0, n_obj - 1] = False
    label = torch.randint(0, L, (B, n_obj), generator=g)
    center = torch.rand((B, n_obj, 2), generator=g) * 1.2 - 0.1  # some centers off the frame
    center[0, 0] = torch.tensor([(H // 2 + 0.3) / H, (W // 2 + 0.6) / W])
    center[0, 1] = torch.tensor([(H // 2 + 0.7) / H, (W // 2 + 0.2) / W])  # the same cell as object 0
    label[0, 1] = label[0, 0]
    if n_obj > 2:
        center[0, 2] = torch.tensor([-0.04, 1.03])  # off the frame, valid
        valid[0, 2] = True
    size = torch.rand((B, n_obj, 2), generator=g) * 0.3
    angle = [torch.rand((B, n_obj), generator=g) * 14 - 7 for _ in range(3)]  # radians, several turns
    depth = torch.rand((B, n_obj), generator=g) * 4 + 0.3
    kvalid = torch.rand((B, n_inst), generator=g) < 0.85
    kvalid[0, :2] = True
    klabel = torch.randint(0, max(K, 1), (B, n_inst), generator=g)
    kcenter = torch.rand((B, n_inst, 2), generator=g)
    kobj = torch.randint(0, n_obj, (B, n_inst), generator=g)
    if c.get("crowd"):  # in sample 1: objects 3..6 in one cell, the first of them invalid; 7 and 8 off the
        for j, (dy, dx) in enumerate(((0.2, 0.7), (0.6, 0.3), (0.8, 0.8), (0.4, 0.5))):  # frame, in one corner cell
            center[1, 3 + j] = torch.tensor([(H // 4 + dy) / H, (W // 4 + dx) / W])
            valid[1, 3 + j] = j > 0
        center[1, 7], center[1, 8] = torch.tensor([1.05, 1.02]), torch.tensor([1.08, 1.06])
        valid[1, 7] = valid[1, 8] = True
    return SimpleNamespace(valid=valid, label=label, center=center, size=size, roll=angle[0], pitch=angle[1],
                           yaw=angle[2], depth=depth, keypoint_valid=kvalid, keypoint_label=klabel,
                           keypoint_center=kcenter, keypoint_object_index=kobj)


def bin_edges(overlap):
    return [pi + overlap / 2, 2 * pi - overlap / 2, pi - overlap / 2, overlap / 2, 0.0, 2 * pi]


def angle_edge_distance(a, modulo, overlap):
    """The distance of each normalised truth angle from the nearest bin edge, in float64."""
    t = (a.double() % modulo) * (2 * pi / modulo)
    return torch.stack([(t - e).abs() for e in bin_edges(overlap)]).min(dim=0).values


def keep_angles_off_edges(truth, c):
    """Move a truth angle whose normalised value is within 0.01 rad of a bin edge by 0.05 of its range."""
    if c["moduli"] is None:
        return
    for a, modulo in zip((truth.roll, truth.pitch, truth.yaw), c["moduli"]):
        for _ in range(4):
            near = angle_edge_distance(a, modulo, c["overlap"]) < ANGLE_BAND
            a[near] += 0.05 * modulo


def cell_edge_distance(center, c):
    """The distance of center * in / ratio from the nearest integer, per coordinate, in float64."""
    v = center.double() * torch.tensor([c["in_h"], c["in_w"]], dtype=torch.float64) / (1 << c["ds"])
    return (v - v.round()).abs()


def keep_centers_off_cell_edges(truth, c):
    """Move a center whose cell coordinate is within 1e-4 of an integer by a hundredth of a cell."""
    step = 0.01 * (1 << c["ds"]) / torch.tensor([c["in_h"], c["in_w"]], dtype=torch.float32)
    for p in (truth.center, truth.keypoint_center):
        for _ in range(4):
            near = cell_edge_distance(p, c) < CELL_BAND
            p[near] += step.expand_as(p)[near]


def make_prediction(c, truth, H, W, g):
    B, L, K = c["B"], len(c["kps"]), sum(c["kps"])
    r = 1 << c["ds"]
    leaf = {"heatmap": 3 * torch.randn((B, L, H, W), generator=g)}
    if K:
        leaf["keypoint_heatmap"] = 3 * torch.randn((B, K, H, W), generator=g)
        leaf["keypoint_affinity"] = torch.randn((B, K, 2, H, W), generator=g)
    widths = {"size": 2, "offset": 2}
    if c["moduli"] is not None:
        for axis in ("roll", "pitch", "yaw"):
            widths[axis + "_bin"] = widths[axis + "_offset"] = 4
    if c["depth"]:
        widths["depth"] = 1
    for name, w in widths.items():
        leaf[name] = torch.randn((B, w, H, W), generator=g)  # NCHW, viewed as NHWC below
    # planted logits on positive cells (object / keypoint centers) and on negative cells
    planted = [20.0, -20.0, 12.0, -12.0, 8.0, -8.0]
    k = 0
    for b in range(B):
        for o in range(c["n_obj"]):
            if truth.valid[b, o]:
                y = int(np.floor(float(truth.center[b, o, 0]) * c["in_h"] / r))
                x = int(np.floor(float(truth.center[b, o, 1]) * c["in_w"] / r))
                if 0 <= y < H and 0 <= x < W:
                    leaf["heatmap"][b, truth.label[b, o], y, x] = planted[k % 6]
                    k += 1
        if K:
            for i in range(c["n_inst"]):
                if truth.keypoint_valid[b, i]:
                    y = int(np.floor(float(truth.keypoint_center[b, i, 0]) * c["in_h"] / r))
                    x = int(np.floor(float(truth.keypoint_center[b, i, 1]) * c["in_w"] / r))
                    leaf["keypoint_heatmap"][b, truth.keypoint_label[b, i], y, x] = planted[k % 6]
                    k += 1
    for name in ("heatmap", "keypoint_heatmap"):
        if name in leaf:
            flat = leaf[name].view(-1)
            cells = torch.randperm(flat.numel(), generator=g)[:12]
            for j, q in enumerate(cells):
                flat[q] = planted[j % 6]
            leaf[name] = out_of_band(leaf[name])
    for t in leaf.values():
        t.requires_grad_(True)
    view = {n: (t if n in ("heatmap", "keypoint_heatmap", "keypoint_affinity") else t.permute(0, 2, 3, 1))
            for n, t in leaf.items()}
    return leaf, view


def train_fields(c):
    """The TrainConfig fields the loss reads."""
    lam = c["lambdas"]
    return dict(heatmap_focal_loss_a=c["focal"][0], heatmap_focal_loss_b=c["focal"][1],
                keypoint_heatmap_sigma=c["sigmas"][0], keypoint_affinity_sigma=c["sigmas"][1],
                loss_lambda_keypoint_heatmap=lam[0], loss_lambda_keypoint_affinity=lam[1],
                loss_lambda_size=lam[2], loss_lambda_offset=lam[3], loss_lambda_angle=lam[4],
                loss_lambda_depth=lam[5])


def moduli_table(c):
    """[3, n_labels] roll, pitch, yaw modulo per label; NaN: None."""
    L = len(c["kps"])
    return np.full((3, L), np.nan) if c["moduli"] is None else np.tile(np.array(c["moduli"])[:, None], (1, L))


def namespaces(in_h, in_w, ds, overlap, fields, moduli, n_keypoints):
    """-> (mc, tc, oc): the model, train and object configs as the loss reads them."""
    r = 1 << ds
    mc = SimpleNamespace(in_h=in_h, in_w=in_w, downsamples=ds, downsample_ratio=r, out_h=in_h // r, out_w=in_w // r,
                         angle_bin_overlap=overlap)
    tc = SimpleNamespace(**fields)
    cfgs = [SimpleNamespace(**{axis: SimpleNamespace(modulo=None if np.isnan(moduli[a, l]) else float(moduli[a, l]))
                               for a, axis in enumerate(("roll", "pitch", "yaw"))}) for l in range(moduli.shape[1])]
    oc = SimpleNamespace(n_labels=moduli.shape[1], n_keypoints=n_keypoints, configs=cfgs)
    return mc, tc, oc


def case_namespaces(c):
    return namespaces(c["in_h"], c["in_w"], c["ds"], c["overlap"], train_fields(c), moduli_table(c), sum(c["kps"]))


def make_inputs(c):
    """-> (truth, leaf, view): the seeded truth namespace and the prediction's leaves (NCHW, requiring grad)
    and views (the reference's shapes) of a case dictionary."""
    g = torch.Generator().manual_seed(c["seed"])
    r = 1 << c["ds"]
    H, W = c["in_h"] // r, c["in_w"] // r
    truth = make_truth(c, H, W, g)
    keep_angles_off_edges(truth, c)
    keep_centers_off_cell_edges(truth, c)
    leaf, view = make_prediction(c, truth, H, W, g)
    return truth, leaf, view


def stored_inputs(c, truth, view):
    """The input arrays a fixture's npz holds: config scalars, truth tensors, `pred_*`."""
    return dict(in_h=c["in_h"], in_w=c["in_w"], downsamples=c["ds"], n_labels=len(c["kps"]), n_keypoints=sum(c["kps"]),
                angle_bin_overlap=c["overlap"], moduli=moduli_table(c),
                **{"tc_" + k: v for k, v in train_fields(c).items()},
                **{k: getattr(truth, k).numpy() for k in TRUTH},
                **{"pred_" + n: v.detach().contiguous().numpy() for n, v in view.items()})


def make_case(c):
    """-> (mc, tc, oc, truth, pred) of a case dictionary, as centernet_loss_ref.load_case returns them: the
    configs as namespaces, the truth as CPU tensors, the prediction as a dict of fp32 CPU tensors in the
    reference's shapes (absent heads None)."""
    truth, _, view = make_inputs(c)
    mc, tc, oc = case_namespaces(c)
    pred = {h: view[h].detach().contiguous() if h in view else None for h in HEADS}
    return mc, tc, oc, truth, pred
