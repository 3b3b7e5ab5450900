"""Test infrastructure of the CenterNet loss (tauv_vision_amd.loss.loss, csrc/loss.hip): a PyTorch-CPU
restatement of the reference's loss (src/tauv_vision/centernet/model/loss.py:138-390) op for op, in the
reference's order, Python loops included, with the targets taken from oracle.ref_targets. In fp32 it
reproduces the reference's values and gradients bit for bit (tests/golden/loss_*.npz, made by
gen_golden_loss.py from the reference itself); in float64 it is the yardstick the device is held to.

Besides each term it returns S, the sum of the absolute values of the elements the term sums (with the
term's lambda and divisor applied): the scale of the tests' tolerances.

Fixture helpers: `load_case(name)` rebuilds a fixture's configs, truth and prediction arrays.
"""
from math import pi
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from helpers import golden
from oracle import ref_targets as rt

HEADS = ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size", "offset", "roll_bin", "roll_offset", "pitch_bin",
         "pitch_offset", "yaw_bin", "yaw_offset", "depth")
TERMS = ("total", "heatmap", "keypoint_heatmap", "keypoint_affinity", "offset", "size", "roll", "pitch", "yaw", "depth",
         "avg_size_error", "max_size_error")
CASES = ("loss_allheads_b2_24x40", "loss_torpedo_b3_23x40", "loss_tiny_b1_5x7", "loss_allheads_b2_24x40_novalid",
         "loss_allheads_b2_24x40_nopositive")


def angle_get_bins(bin_overlap):
    return (pi / 2, -bin_overlap / 2, pi + bin_overlap / 2), (-pi / 2, -pi - bin_overlap / 2, bin_overlap / 2)


def angle_range(label, oc, axis):
    B, n = label.shape
    out = torch.zeros_like(label, dtype=torch.float32)
    for b in range(B):
        for o in range(n):
            modulo = getattr(oc.configs[label[b, o]], axis).modulo
            if modulo is not None:
                out[b, o] = modulo
    return out


def focal_loss(prediction, truth, alpha, beta):
    """-> (elementwise loss, N)"""
    p = torch.isclose(truth, torch.ones(1, dtype=truth.dtype, device=truth.device))
    N = torch.sum(p)
    pf = p.to(prediction.dtype)
    loss_p = ((1 - prediction) ** alpha) * torch.log(torch.clamp(prediction, min=1e-4)) * pf
    loss_n = ((1 - truth) ** beta) * (prediction ** alpha) * torch.log(torch.clamp(1 - prediction, min=1e-4)) * (1 - pf)
    if N == 0:
        return -loss_p, N
    return -(loss_p + loss_n) / N, N


def angle_in_range(angles, range_min, range_max):
    range_min = range_min % (2 * pi)
    range_max = range_max % (2 * pi)
    angles = angles % (2 * pi)
    if range_min < range_max:
        return (range_min <= angles) & (angles <= range_max)
    return (range_min <= angles) | (angles <= range_max)


def angle_loss(predicted_bin, predicted_offset, truth, theta_range, bin_overlap):
    B, n = truth.shape
    truth = truth % theta_range
    truth = truth * (2 * pi / theta_range)
    (c0, lo0, hi0), (c1, lo1, hi1) = angle_get_bins(bin_overlap)
    in0 = angle_in_range(truth, lo0, hi0).to(torch.long)
    in1 = angle_in_range(truth, lo1, hi1).to(torch.long)
    off0 = torch.stack((torch.sin(truth - c0), torch.cos(truth - c0)), dim=-1)
    off1 = torch.stack((torch.sin(truth - c1), torch.cos(truth - c1)), dim=-1)
    cls0 = F.cross_entropy(predicted_bin[:, :, 0:2].reshape(-1, 2), in0.reshape(-1), reduction="none")
    cls1 = F.cross_entropy(predicted_bin[:, :, 2:4].reshape(-1, 2), in1.reshape(-1), reduction="none")
    l0 = F.l1_loss(predicted_offset[:, :, 0:2].reshape(-1, 2), off0.reshape(-1, 2), reduction="none").sum(dim=-1)
    l1 = F.l1_loss(predicted_offset[:, :, 2:4].reshape(-1, 2), off1.reshape(-1, 2), reduction="none").sum(dim=-1)
    result = (cls0 + cls1
              + in0.reshape(-1).to(predicted_bin.dtype) * l0
              + in1.reshape(-1).to(predicted_bin.dtype) * l1)
    return result.reshape(B, n)


def depth_loss(prediction, truth):
    B, n = truth.shape
    return F.l1_loss(1 / torch.sigmoid(prediction.reshape(-1)) - 1, truth.reshape(-1), reduction="none").reshape(B, n)


def _s(el):
    return float(el.detach().abs().sum())


def loss_ref(pred, truth, mc, tc, oc, dtype=torch.float32):
    """pred: namespace of CPU tensors of `dtype` in the reference's shapes (absent heads None); truth: the
    fixture's tensors (fp32 / int64 / bool). -> (terms, S): dicts by TERMS name (absent terms missing).
    Everything may live on a GPU (the timing baseline of tools/centernet_loss_bench.py): the oracle builds
    the targets on the host and they are moved to the prediction's device, the rest runs there."""
    dev = pred.heatmap.device
    f = lambda t: t.to(device=dev, dtype=dtype)  # noqa: E731
    terms, S = {}, {}
    host = truth if dev.type == "cpu" else SimpleNamespace(**{k: v if v is None else v.cpu() for k, v in vars(truth).items()})
    heatmap = f(rt.generate_heatmap(host, mc, tc, oc.n_labels))
    if pred.keypoint_heatmap is not None:
        kh, kw, ka = (f(t) for t in rt.generate_keypoint_heatmap(host, mc, tc, oc.n_keypoints))
    out_index = rt.out_index_for_position(truth.center, mc)
    B, n, _ = out_index.shape
    center, size, valid = f(truth.center), f(truth.size), truth.valid

    gathered = {}
    for name in HEADS[3:]:
        if getattr(pred, name) is not None:
            width = () if name == "depth" else (2,) if name in ("size", "offset") else (4,)
            gathered[name] = torch.zeros((B, n) + width, dtype=dtype, device=dev)
    for b in range(B):
        for o in range(n):
            for name in gathered:
                v = getattr(pred, name)[b, out_index[b, o, 0], out_index[b, o, 1]]
                gathered[name][b, o] = v.reshape(()) if name == "depth" else v

    n_valid = min(int(valid.to(torch.float32).sum()), 1)

    el, _ = focal_loss(torch.sigmoid(pred.heatmap), heatmap, tc.heatmap_focal_loss_a, tc.heatmap_focal_loss_b)
    l_heat = el.sum()
    S["heatmap_alone"] = _s(el)
    terms["heatmap_alone"] = l_heat.detach().clone()
    total = l_heat
    s_total = S["heatmap_alone"]

    def add(name, value, s):
        nonlocal total, s_total
        terms[name], S[name] = value, float(s)
        total = total + value
        s_total += float(s)

    if pred.keypoint_heatmap is not None:
        el, _ = focal_loss(torch.sigmoid(pred.keypoint_heatmap), kh, tc.heatmap_focal_loss_a, tc.heatmap_focal_loss_b)
        add("keypoint_heatmap", tc.loss_lambda_keypoint_heatmap * el.sum(),
            tc.loss_lambda_keypoint_heatmap * _s(el))
    if pred.keypoint_affinity is not None:
        el = kw.unsqueeze(2) * F.mse_loss(pred.keypoint_affinity, ka, reduction="none")
        add("keypoint_affinity", tc.loss_lambda_keypoint_affinity * el.sum(),
            tc.loss_lambda_keypoint_affinity * _s(el))

    inv = 1.0 / n_valid if n_valid else float("nan")  # no valid object: the term is NaN and has no scale

    el = valid.unsqueeze(-1) * F.l1_loss(gathered["size"], size, reduction="none")
    add("size", tc.loss_lambda_size * el.sum() / n_valid, tc.loss_lambda_size * _s(el) * inv)
    size_error = torch.where(valid.unsqueeze(-1), torch.abs(gathered["size"] - size), torch.nan)
    terms["avg_size_error"] = size_error.nanmean()
    terms["max_size_error"] = torch.where(torch.isnan(size_error), 0, size_error).max()
    S["avg_size_error"] = S["max_size_error"] = float(terms["max_size_error"].detach())  # the largest element

    pixel_center = center * torch.Tensor((mc.in_h, mc.in_w)).to(dev).unsqueeze(0).unsqueeze(1)
    pixel_offset = pixel_center - mc.downsample_ratio * (pixel_center / mc.downsample_ratio).to(torch.long)
    el = valid.unsqueeze(-1) * F.l1_loss(gathered["offset"], pixel_offset, reduction="none")
    add("offset", tc.loss_lambda_offset * el.sum() / n_valid, tc.loss_lambda_offset * _s(el) * inv)

    for axis in ("roll", "pitch", "yaw"):
        if getattr(pred, axis + "_bin") is None:
            continue
        theta_range = f(angle_range(truth.label, oc, axis))
        el = angle_loss(gathered[axis + "_bin"], gathered[axis + "_offset"], f(getattr(truth, axis)), theta_range,
                        mc.angle_bin_overlap)
        l = el.sum()
        add(axis, tc.loss_lambda_angle * (valid * l).sum() / n_valid,
            tc.loss_lambda_angle * float(valid.sum()) * _s(el) * inv)
    if pred.depth is not None:
        el = valid * depth_loss(gathered["depth"], f(truth.depth))
        add("depth", tc.loss_lambda_depth * el.sum() / n_valid, tc.loss_lambda_depth * _s(el) * inv)

    terms["total"] = terms["heatmap"] = total
    S["total"] = S["heatmap"] = s_total
    return terms, S


# ---- fixtures -------------------------------------------------------------------------------------

def base_name(name):
    """The fixture that holds a case's inputs (the derived cases D and E store only what differs)."""
    for suffix in ("_novalid", "_nopositive"):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def load_case(name):
    """-> (g, mc, tc, oc, truth, pred arrays): g the case's npz (values `val_*`, gradients `grad_*`), the
    configs as namespaces, the truth as CPU tensors, the prediction as a dict of fp32 CPU tensors in the
    reference's shapes (absent heads None)."""
    g, base = golden(name), golden(base_name(name))
    t = lambda k: torch.from_numpy(base[k])  # noqa: E731
    ds = int(base["downsamples"])
    r = 1 << ds
    mc = SimpleNamespace(in_h=int(base["in_h"]), in_w=int(base["in_w"]), downsamples=ds, downsample_ratio=r,
                         out_h=int(base["in_h"]) // r, out_w=int(base["in_w"]) // r,
                         angle_bin_overlap=float(base["angle_bin_overlap"]))
    tc = SimpleNamespace(**{k[3:]: float(base[k]) for k in base.files if k.startswith("tc_")})
    moduli = base["moduli"]  # [3, n_labels] roll, pitch, yaw; NaN: None
    cfgs = [SimpleNamespace(**{axis: SimpleNamespace(modulo=None if np.isnan(moduli[a, l]) else float(moduli[a, l]))
                               for a, axis in enumerate(("roll", "pitch", "yaw"))}) for l in range(moduli.shape[1])]
    oc = SimpleNamespace(n_labels=int(base["n_labels"]), n_keypoints=int(base["n_keypoints"]), configs=cfgs)
    truth = SimpleNamespace(**{k: t(k) for k in ("valid", "label", "center", "size", "roll", "pitch", "yaw", "depth",
                                                 "keypoint_valid", "keypoint_label", "keypoint_center",
                                                 "keypoint_object_index")})
    if name.endswith("_novalid"):
        truth.valid = torch.zeros_like(truth.valid)
    if name.endswith("_nopositive"):
        truth.keypoint_valid = torch.zeros_like(truth.keypoint_valid)
    pred = {h: t("pred_" + h) if "pred_" + h in base.files else None for h in HEADS}
    return g, mc, tc, oc, truth, pred


def leaves(pred, dtype):
    """The prediction dict as a namespace of leaf tensors of `dtype` that require grad."""
    return SimpleNamespace(**{h: None if v is None else v.to(dtype).clone().requires_grad_(True)
                              for h, v in pred.items()})
