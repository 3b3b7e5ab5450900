"""Golden fixtures for the CenterNet loss (reference loss.py:178-390).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's loss.py (through
gen_golden_targets._import_reference), builds seeded truth batches and synthetic predictions in the
reference model's layout (NCHW heatmaps, NHWC views of NCHW heads) by the recipe of
tests/centernet_loss_cases.py (the case dictionaries, the conditions on the inputs), runs the reference's
loss() and total.backward() in fp32 on the CPU, and stores the inputs, every term's value and every
prediction tensor's gradient as tests/golden/loss_*.npz. Data only: the reference source does not travel.
    python tests/golden/gen_golden_loss.py
"""
import os
import sys
import types

import numpy as np
import torch

from gen_golden_targets import _import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from centernet_loss_cases import CASES, HEADS, TRUTH, make_inputs, stored_inputs, train_fields  # noqa: E402

TERMS = ("total", "heatmap", "keypoint_heatmap", "keypoint_affinity", "offset", "size", "roll", "pitch", "yaw", "depth",
         "avg_size_error", "max_size_error")


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
        mc = rcfg.ModelConfig([2] * 5, [16] * 6, c["in_h"], c["in_w"], c["ds"], c["overlap"])
        tc = rcfg.TrainConfig(lr=1e-3, batch_size=c["B"], n_batches=1, n_epochs=1, heatmap_sigma_factor=0.05,
                              n_workers=0, weight_save_interval=1, **train_fields(c))
        L, K = len(c["kps"]), sum(c["kps"])
        cfgs = [types.SimpleNamespace(**{axis: types.SimpleNamespace(modulo=None if c["moduli"] is None else c["moduli"][a])
                                         for a, axis in enumerate(("roll", "pitch", "yaw"))}) for _ in range(L)]
        oc = types.SimpleNamespace(n_labels=L, n_keypoints=K, configs=cfgs)
        fields, leaf, view = make_inputs(c)
        truth = rpose.PoseSample(img=torch.zeros((c["B"], 3, 1, 1)), **{k: getattr(fields, k) for k in TRUTH})
        res = run(rloss, rcfg, c, truth, view, leaf, mc, tc, oc)
        inputs = stored_inputs(c, truth, view)
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
