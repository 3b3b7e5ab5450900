"""YOLACT training loss: tauv_vision_amd.yolact_loss.loss against the reference's algorithm on the same GPU.

Workload: the 550 x 550 geometry of tools/yolact_full_bench.py (pyramid 69, 35, 18, 9, 5, anchor scales
24 .. 384, 138 x 138 prototypes, a 550 x 550 seg map), B = 8, T = 12 seeded truths per sample (jittered
anchors, so each has a few positives; an ellipse per truth in the seg map, a stripe of invalid image), a
synthetic fp32 prediction in the reference model's layout. Two shapes:
  bench     the configuration yolact_full_bench.py runs: one aspect ratio (A = 6 416), C = 7, P = 8;
  product   three aspect ratios (A = 19 248), C = 7, P = 32.
One step is loss(...) and total.backward(), wall time between two device synchronisations.
  baseline  tests/yolact_loss_ref.py's loss_ref on fp32 CUDA tensors: the reference's own sequence of
            torch ops and Python loops (per sample, and per positive anchor with its host round trip),
            keeping no record;
  new       tauv_vision_amd.yolact_loss.loss on the same tensors.
Three alternating rounds of `--steps` steps after `--warmup`; a round's figure is its median, a side's the
median of its three rounds, `*_spread_ms` is max - min of a side's three. The values of the two sides are
compared (relative difference of each term) so that the times are of the same computation. Prints one
line per figure and a final JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time
from math import sqrt
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yolact_loss_cases as C  # noqa: E402
import yolact_loss_ref as R  # noqa: E402
from tauv_vision_amd import _lib, yolact_loss as L  # noqa: E402

IN, LEVELS, SCALES, PROTO, T = 550, ((69, 69), (35, 35), (18, 18), (9, 9), (5, 5)), (24, 48, 96, 192, 384), 138, 12
SHAPES = {"bench": dict(ars=(1.0,), C=7, P=8), "product": dict(ars=(1.0, 0.5, 2.0), C=7, P=32)}


def make_case(shape, B, dev, seed=41):
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    cfg = SimpleNamespace(in_h=IN, in_w=IN, anchor_scales=SCALES, anchor_aspect_ratios=s["ars"], box_variances=(0.1, 0.2),
                          iou_pos_threshold=0.5, iou_neg_threshold=0.4, negative_example_ratio=3)
    anchor = torch.cat([C.get_anchor(i, sz, cfg) for i, sz in enumerate(LEVELS)], dim=1).contiguous()
    A = anchor.shape[1]
    # truths from the three coarser levels' anchors (objects of 96 .. 384 pixels), jittered
    first = sum(h * w for h, w in LEVELS[:2]) * len(s["ars"])
    pick = torch.randint(first, A, (B, T), generator=g)
    base = anchor[0][pick]
    jitter = (torch.rand((B, T, 2), generator=g) - 0.5) * 0.3
    grow = torch.exp((torch.rand((B, T, 2), generator=g) - 0.5) * 0.3)
    box = torch.cat((base[..., :2] + jitter * base[..., 2:], base[..., 2:] * grow), dim=-1).contiguous()
    valid = torch.ones((B, T), dtype=torch.bool)
    valid[:, -1] = False
    cls = torch.randint(1, s["C"], (B, T), generator=g).to(torch.uint8)
    seg = torch.full((B, IN, IN), C.BACKGROUND, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(IN) + 0.5, torch.arange(IN) + 0.5, indexing="ij")
    for b in range(B):
        for t in range(T):
            cy, cx, bh, bw = (float(v) * IN for v in box[b, t])
            seg[b][((yy - cy) / (bh / 2)) ** 2 + ((xx - cx) / (bw / 2)) ** 2 <= 1.0] = t
    img_valid = torch.ones((B, IN, IN), dtype=torch.bool)
    img_valid[:, :, 200:230] = False
    pred = (2.0 * torch.randn((B, A, s["C"]), generator=g), 1.5 * torch.randn((B, A, 4), generator=g),
            torch.tanh(torch.randn((B, A, s["P"]), generator=g)), anchor,
            (3.3 / sqrt(s["P"])) * torch.relu(torch.randn((B, s["P"], PROTO, PROTO), generator=g)))
    pred = tuple(t.to(dev).requires_grad_(i != 3) for i, t in enumerate(pred))
    truth = tuple(t.to(dev) for t in (valid, cls, box, seg, img_valid))
    return cfg, pred, truth


def step_ms(fn, pred, steps, warmup):
    times = []
    for i in range(warmup + steps):
        for t in pred:
            t.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn().backward()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def count_launches(fn):
    """The library calls of one step that launch (every call's status goes through _lib.check; the
    workspace-size query does not launch)."""
    n, check = [0], _lib.check
    _lib.check = lambda rc, what="": (n.__setitem__(0, n[0] + 1), check(rc, what))[1]
    try:
        fn().backward()
        torch.cuda.synchronize()
    finally:
        _lib.check = check
    return n[0] - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="bench,product")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "yolact_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yolact_loss_bench needs the MI355X: no HIP device is visible")
    dev = torch.device("cuda", 0)
    res = {"tool": "yolact_loss_bench", "input": [IN, IN], "prototypes": [PROTO, PROTO], "truths": T, "batch": a.batch,
           "steps": []}
    for shape in a.shapes.split(","):
        cfg, pred, truth = make_case(shape, a.batch, dev)
        long_truth = (truth[0], truth[1].long(), *truth[2:])  # F.cross_entropy takes int64 targets
        new = lambda: L.loss(pred, truth, cfg)[0]  # noqa: E731
        base = lambda: R.loss_ref(pred, long_truth, cfg, record=False)[0]["total"]  # noqa: E731
        with torch.no_grad():
            total, terms, state = L.loss_with_state(pred, truth, cfg)
            ref = R.loss_ref(pred, long_truth, cfg, record=False)[0]
        dev_vals = dict(zip(R.TERMS, (total,) + tuple(terms)))
        rel = {t: abs(float(dev_vals[t]) - float(ref[t])) / max(abs(float(ref[t])), 1e-30) for t in R.TERMS}
        rounds = {"baseline": [], "new": []}
        for _ in range(3):
            rounds["baseline"].append(step_ms(base, pred, a.steps, a.warmup))
            rounds["new"].append(step_ms(new, pred, 4 * a.steps, a.warmup + 2))
        row = {"shape": shape, "B": a.batch, "A": pred[0].shape[1], "C": pred[0].shape[2], "P": pred[2].shape[2],
               "steps": a.steps, "warmup": a.warmup, "total": float(total),
               "positives_per_sample": [int(v) for v in state.positive.sum(dim=1).cpu()],
               "selected_per_sample": [int(v) for v in state.selected.sum(dim=1).cpu()],
               "launches_per_step": count_launches(new), "relative_difference": rel}
        for side, v in rounds.items():
            row[side + "_ms"] = float(np.median(v))
            row[side + "_rounds_ms"] = v
            row[side + "_spread_ms"] = max(v) - min(v)
        row["ratio"] = row["baseline_ms"] / row["new_ms"]
        row["ok"] = row["new_ms"] <= row["baseline_ms"] + row["baseline_spread_ms"] and max(rel.values()) < 1e-4
        print(f"{shape}: A {row['A']} P {row['P']} positives {sum(row['positives_per_sample'])} baseline "
              f"{row['baseline_ms']:.2f} ms new {row['new_ms']:.3f} ms ratio {row['ratio']:.1f} launches "
              f"{row['launches_per_step']} worst relative difference {max(rel.values()):.2e}")
        res["steps"].append(row)
    res["ok"] = all(r["ok"] for r in res["steps"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
