"""Test infrastructure of the CenterNet loss (tauv_vision_amd.loss.loss, csrc/loss.hip): a PyTorch-CPU
restatement of the reference's loss (src/tauv_vision/centernet/model/loss.py:138-390) op for op, in the
reference's order, Python loops included, with the targets taken from oracle.ref_targets. In fp32 it
reproduces the reference's values and gradients bit for bit (tests/golden/loss_*.npz, made by
gen_golden_loss.py from the reference itself); in float64 it is the yardstick the device is held to.

Besides each term it returns S, the sum of the absolute values of the elements the term sums (with the
term's lambda and divisor applied): the scale of the tests' tolerances.

Case helpers: `load_case(name)` rebuilds a fixture's configs, truth and prediction arrays; `case_inputs`
does the same for a fixture or a generated case (centernet_loss_cases.GENERATED, no stored results);
`restated` runs the restatement in float64 and fp32 once per case; `check_values` / `check_grads` are the
tolerance rule of the GPU tests (test_gpu_centernet_loss.py states it), in plain numpy.
"""
import functools
from math import pi
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import centernet_loss_cases as C
from centernet_loss_cases import HEADS
from helpers import golden
from oracle import ref_targets as rt

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
    mc, tc, oc = C.namespaces(int(base["in_h"]), int(base["in_w"]), int(base["downsamples"]),
                              float(base["angle_bin_overlap"]),
                              {k[3:]: float(base[k]) for k in base.files if k.startswith("tc_")},
                              base["moduli"], int(base["n_keypoints"]))
    assert oc.n_labels == int(base["n_labels"])
    truth = SimpleNamespace(**{k: t(k) for k in C.TRUTH})
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


def case_inputs(name):
    """-> (g, mc, tc, oc, truth, pred) of a fixture (load_case) or of a generated case (g None)."""
    if name in C.GENERATED:
        return (None,) + C.make_case(C.GENERATED[name])
    return load_case(name)


def _numpy(d):
    return {k: v.detach().double().cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def restated(name, rounding=torch.float32):
    """(values64, S, grads64, values32, grads32) of a case, the prediction rounded to `rounding` first. The
    fp32 side of a fixture in fp32 is the reference's own stored results, else the fp32 restatement. The
    results are shared between the tests: they are not to be modified."""
    g, mc, tc, oc, truth, pred = case_inputs(name)
    pred = {h: None if v is None else v.to(rounding).float() for h, v in pred.items()}
    out = []
    for dtype in (torch.float64, torch.float32):
        p = leaves(pred, dtype)
        terms, S = loss_ref(p, truth, mc, tc, oc, dtype)
        terms["total"].backward()
        out += [_numpy(terms), S, {h: getattr(p, h).grad.double().numpy() for h in HEADS if pred[h] is not None}]
    v64, S, g64, v32, _, g32 = out
    if g is not None and rounding == torch.float32:  # the reference's own fp32 results
        v32 = {t: g["val_" + t].astype(np.float64) for t in TERMS if "val_" + t in g.files}
        g32 = {h: g["grad_" + h].astype(np.float64) for h in g64}
    return v64, S, g64, v32, g32


FLOOR = 2.0 ** -20


def check_values(dev, v64, S, v32):
    """-> the worst error over its tolerance."""
    worst = 0.0
    for t, want in v64.items():
        if t == "heatmap_alone":
            continue
        if np.isnan(want) or np.isnan(v32[t]):
            assert np.isnan(want) and np.isnan(v32[t]) and np.isnan(dev[t]), t
            continue
        e_ref = abs(v32[t] - want) / S[t] if S[t] else 0.0
        tol = max(4 * e_ref, FLOOR) * S[t]
        print(f"{t}: dev {dev[t]:.9g} f64 {want:.9g} err {abs(dev[t] - want):.3g} tol {tol:.3g} e_ref {e_ref:.3g}")
        assert abs(dev[t] - want) <= tol, (t, dev[t], want, tol)
        if tol:
            worst = max(worst, float(abs(dev[t] - want) / tol))
    return worst


def check_grads(dev, g64, g32, half=0.0):
    """-> the worst error over its bound."""
    worst = 0.0
    for h, want in g64.items():
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(g32[h]), nan, err_msg=h)
        np.testing.assert_array_equal(np.isnan(dev[h]), nan, err_msg=h)
        w, d, r = want[~nan], dev[h][~nan], g32[h][~nan]
        if w.size == 0:
            continue
        bound = max(4 * np.abs(r - w).max(), FLOOR * np.abs(w).max())
        err = np.abs(d - w)
        print(f"grad {h}: max err {err.max():.3g} bound {bound:.3g} max |g64| {np.abs(w).max():.3g}")
        assert (err <= bound + half * np.abs(w)).all(), (h, float((err - half * np.abs(w)).max()), bound)
        if bound:
            worst = max(worst, float((err / (bound + half * np.abs(w))).max()))
    return worst
