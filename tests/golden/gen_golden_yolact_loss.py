"""Golden fixtures for the YOLACT loss (reference yolact/model/loss.py:8-124).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's loss.py, draws each case's inputs
by the recipe of tests/yolact_loss_cases.py (the case dictionaries, the seeds, the conditions on the
inputs), runs the reference's loss() and total.backward() in fp32 on the CPU with plain torch, and stores
the inputs, the four values, the four gradients and the reference's intermediate sets as
tests/golden/yolact_loss_*.npz. Data only: the reference source does not travel.

The sets are read off the reference's own calls: iou_matrix and torch.topk are wrapped while loss() runs
(the wrappers return what the wrapped functions return), so match_index / positive / negative come from
the reference's iou and the selected set from its topk indices.
    python tests/golden/gen_golden_yolact_loss.py
"""
import os
import sys

import numpy as np
import torch

from gen_golden_targets import REF_SRC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import yolact_loss_cases as C  # noqa: E402


def run(rloss, inputs, cfg):
    pred = tuple(inputs[k].clone().requires_grad_(k != "anchor") for k in C.PREDICTION)
    truth = tuple(inputs[k].clone() for k in C.TRUTH)
    seen = {"iou": None, "topk": []}
    iou_matrix, topk = rloss.iou_matrix, torch.topk

    def spy_iou(a, b):
        seen["iou"] = iou_matrix(a, b)
        return seen["iou"]

    def spy_topk(x, k, *a, **kw):
        out = topk(x, k, *a, **kw)
        seen["topk"].append(out[1].detach().clone())
        return out
    rloss.iou_matrix, torch.topk = spy_iou, spy_topk
    try:
        total, terms = rloss.loss(pred, truth, cfg)
    finally:
        rloss.iou_matrix, torch.topk = iou_matrix, topk
    total.backward()
    match_iou, match_index = torch.max(seen["iou"].detach() * truth[0].unsqueeze(1).float(), dim=2)
    positive = match_iou >= cfg.iou_pos_threshold
    negative = match_iou <= cfg.iou_neg_threshold
    selected = positive.clone()
    for b, idx in enumerate(seen["topk"]):
        selected[b, idx] = True
    out = {"val_" + n: v.detach().numpy().copy() for n, v in zip(("total", "classification", "box", "mask"),
                                                                  (total,) + tuple(terms))}
    for k, t in zip(C.PREDICTION, pred):
        if k != "anchor":
            out["grad_" + k] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().copy()
    out["match_index"] = torch.where(positive, match_index, -1).to(torch.int32).numpy()  # -1: not compared
    out["positive"], out["negative"], out["selected"] = (t.to(torch.uint8).numpy() for t in (positive, negative, selected))
    return out


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_SRC)
    from tauv_vision.yolact.model import loss as rloss
    for name, c in C.CASES.items():
        inputs = C.make_inputs(c)
        res = run(rloss, inputs, C.config_of(c))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), seed=np.int64(c["seed"]), **C.stored(inputs), **res)
        print(name, {k: float(v) for k, v in res.items() if k.startswith("val_")},
              "positives", int(res["positive"].sum()), "selected", int(res["selected"].sum()))


if __name__ == "__main__":
    main()
