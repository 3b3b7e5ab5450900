"""Golden fixtures for the CenterNet loss (reference loss.py:178-390).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's loss.py (through
gen_golden_targets._import_reference), builds seeded truth batches and synthetic predictions in the
reference model's layout (NCHW heatmaps, NHWC views of NCHW heads), runs the reference's loss() and
total.backward() in fp32 on the CPU, and stores the inputs, every term's value and every prediction
tensor's gradient as tests/golden/loss_*.npz. Data only: the reference source does not travel.
    python tests/golden/gen_golden_loss.py

Conditions on the inputs (not tolerances):
  * no heatmap / keypoint-heatmap logit z, as fp32, fp16 or bf16, has | |z| - ln 9999 | < 0.05: there
    sigmoid or 1 - sigmoid sits at focal_loss's 1e-4 clamp, whose gradient is discontinuous, so fp32
    and float64 legitimately disagree by O(1) on such an element;
  * no normalised truth angle lies within 0.01 rad of a bin edge (bin membership is a step).
"""
import os
import types
from math import log, pi

import numpy as np
import torch

from gen_golden_targets import _import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
HEADS = ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size", "offset", "roll_bin", "roll_offset", "pitch_bin",
         "pitch_offset", "yaw_bin", "yaw_offset", "depth")
TERMS = ("total", "heatmap", "keypoint_heatmap", "keypoint_affinity", "offset", "size", "roll", "pitch", "yaw", "depth",
         "avg_size_error", "max_size_error")
CLAMP_Z = log(9999.0)

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


def out_of_band(z):
    bad = torch.zeros_like(z, dtype=torch.bool)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        bad |= (z.to(dt).float().abs() - CLAMP_Z).abs() < 0.05
    return torch.where(bad, torch.sign(z) * (CLAMP_Z + 0.25), z)


def make_truth(rpose, c, H, W, g):
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
    return rpose.PoseSample(img=torch.zeros((B, 3, 1, 1)), valid=valid, label=label, center=center, size=size,
                            roll=angle[0], pitch=angle[1], yaw=angle[2], depth=depth, keypoint_valid=kvalid,
                            keypoint_label=klabel, keypoint_center=kcenter, keypoint_object_index=kobj)


def keep_angles_off_edges(truth, c):
    """Move a truth angle whose normalised value is within 0.01 rad of a bin edge by 0.05 of its range."""
    if c["moduli"] is None:
        return
    ov = c["overlap"]
    edges = [pi + ov / 2, 2 * pi - ov / 2, pi - ov / 2, ov / 2, 0.0, 2 * pi]
    for a, modulo in zip((truth.roll, truth.pitch, truth.yaw), c["moduli"]):
        for _ in range(4):
            t = (a.double() % modulo) * (2 * pi / modulo)
            near = torch.zeros_like(a, dtype=torch.bool)
            for e in edges:
                near |= (t - e).abs() < 0.01
            a[near] += 0.05 * modulo


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


def run(rloss, rcfg, c, truth, view, leaf, mc, tc, oc):
    for t in leaf.values():
        t.grad = None
    pred = rloss.Prediction(**{h: view.get(h) for h in HEADS})
    losses = rloss.loss(pred, truth, mc, tc, oc, None)
    losses.total.backward()
    out = {}
    for name in TERMS:
        v = getattr(losses, name)
        if v.dim() == 0:  # the dataclass default (a 1-element zeros) marks an absent term
            out["val_" + name] = v.detach().numpy().copy()
    for n, t in leaf.items():
        gr = t.grad if n in ("heatmap", "keypoint_heatmap", "keypoint_affinity") else t.grad.permute(0, 2, 3, 1)
        out["grad_" + n] = gr.contiguous().numpy().copy()
    return out


def main():
    rcfg, rloss, rpose = _import_reference()
    for name, c in CASES.items():
        g = torch.Generator().manual_seed(c["seed"])
        mc = rcfg.ModelConfig([2] * 5, [16] * 6, c["in_h"], c["in_w"], c["ds"], c["overlap"])
        H, W = mc.out_h, mc.out_w
        lam = c["lambdas"]
        tc_fields = dict(heatmap_focal_loss_a=c["focal"][0], heatmap_focal_loss_b=c["focal"][1],
                         keypoint_heatmap_sigma=c["sigmas"][0], keypoint_affinity_sigma=c["sigmas"][1],
                         loss_lambda_keypoint_heatmap=lam[0], loss_lambda_keypoint_affinity=lam[1],
                         loss_lambda_size=lam[2], loss_lambda_offset=lam[3], loss_lambda_angle=lam[4],
                         loss_lambda_depth=lam[5])
        tc = rcfg.TrainConfig(lr=1e-3, batch_size=c["B"], n_batches=1, n_epochs=1, heatmap_sigma_factor=0.05,
                              n_workers=0, weight_save_interval=1, **tc_fields)
        L, K = len(c["kps"]), sum(c["kps"])
        moduli = np.full((3, L), np.nan) if c["moduli"] is None else np.tile(np.array(c["moduli"])[:, None], (1, L))
        cfgs = [types.SimpleNamespace(**{axis: types.SimpleNamespace(modulo=None if c["moduli"] is None else c["moduli"][a])
                                         for a, axis in enumerate(("roll", "pitch", "yaw"))}) for _ in range(L)]
        oc = types.SimpleNamespace(n_labels=L, n_keypoints=K, configs=cfgs)
        truth = make_truth(rpose, c, H, W, g)
        keep_angles_off_edges(truth, c)
        leaf, view = make_prediction(c, truth, H, W, g)
        res = run(rloss, rcfg, c, truth, view, leaf, mc, tc, oc)
        inputs = dict(in_h=c["in_h"], in_w=c["in_w"], downsamples=c["ds"], n_labels=L, n_keypoints=K,
                      angle_bin_overlap=c["overlap"], moduli=moduli,
                      **{"tc_" + k: v for k, v in tc_fields.items()},
                      **{k: getattr(truth, k).numpy() for k in ("valid", "label", "center", "size", "roll", "pitch",
                                                                "yaw", "depth", "keypoint_valid", "keypoint_label",
                                                                "keypoint_center", "keypoint_object_index")},
                      **{"pred_" + n: v.detach().contiguous().numpy() for n, v in view.items()})
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **inputs, **res)
        print(name, {k: float(v) for k, v in res.items() if k.startswith("val_")})
        if name == "loss_allheads_b2_24x40":
            keep = {k: getattr(truth, k).clone() for k in ("valid", "keypoint_valid")}
            for suffix, field in (("_novalid", "valid"), ("_nopositive", "keypoint_valid")):
                setattr(truth, field, torch.zeros_like(keep[field]))
                res = run(rloss, rcfg, c, truth, view, leaf, mc, tc, oc)
                setattr(truth, field, keep[field])
                np.savez_compressed(os.path.join(HERE, name + suffix + ".npz"), **res)
                print(name + suffix, {k: float(v) for k, v in res.items() if k.startswith("val_")})


if __name__ == "__main__":
    main()
