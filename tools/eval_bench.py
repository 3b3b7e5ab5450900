"""Precision-recall curve of a detector over a data set: the one-pass device evaluation against the
reference's procedure restated on this package's own API.

Workload: the R18 golden model (r18_c128_b1_480x640's backbone, seeded weights, fp16) at 360 x 640, a
synthetic loader of 16 batches of 8 seeded images already on the device, 8 truths per image planted from
the model's own decode (so that the matching has work), ten score thresholds spread over the scores the
seeded model gives. iou_threshold 0: a seeded model's size head gives boxes of negative size, which overlap
nothing, so a positive threshold would match nothing and both curves would be zero; at 0 the reference lets
every pair of equal labels pass (its quirk, kept), the match test is still evaluated for every pair, and
the truths are contended for.

  one_pass   tv.evaluate_precision_recall_curve: per batch the native forward, one DeviceDecoder call at
             K = 100 and the lowest threshold, one tv_evaluate_detections launch; one device-to-host copy
             at the end.
  ten_pass   the reference's evaluate_precision_recall_curve (evaluate.py:211-233) on our API: for every
             threshold a pass over the loader with the native forward, tv.decode to Python Detection
             lists, and the host matching of tests/eval_ref.py.
Wall time of the whole curve, the device idle before and after; one warm-up of each, then --rounds
alternating rounds of one ten_pass run and --inner one_pass runs; every sample, the medians and min / max
are written. Both must give the same curve. The launch counts come from a torch.profiler trace of the
one-pass path: the kernels of one batch by name, and the device-to-host copies of a whole curve. The tool
FAILS unless the curves are equal, one batch launches exactly one evaluation kernel beyond forward and
decode, and a data set makes exactly one device-to-host copy — or if the profiler gives no device events.
Prints a JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_ref  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402
from recipe import case_by_name, seeded_state_dict  # noqa: E402

IN_H, IN_W, BATCHES, B, N, IOU = 360, 640, 16, 8, 8, 0.0


class Batch:
    def __init__(self, img, valid, label, center, size):
        self.img, self.valid, self.label, self.center, self.size = img, valid, label, center, size

    def to(self, device):
        return self


def build(dev):
    case = case_by_name("r18_c128_b1_480x640")
    o = case["objects"]
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, 1.0), A(False, 1.0), A(False, 1.0), False, False, None)
                             for i in range(o["n_labels"])])
    model = tv.Centernet(tv.DLABackbone(case["heights"], case["channels"], case["downsamples"]), oc, precision="fp16")
    model.load_state_dict(seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()]))
    mc = tv.ModelConfig(case["heights"], case["channels"], IN_H, IN_W, case["downsamples"], 1.0)
    return model.to(dev).eval(), mc


def make_loader(model, mc, dev):
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(5)
    loader, scores = [], []
    for _ in range(BATCHES):
        img = torch.randn((B, 3, IN_H, IN_W), generator=g).to(dev)
        with torch.no_grad():
            rec, cnt = tv.decode_records(model(img), mc, 100, 0.0)
        pick = np.stack([rng.choice(int(c), size=N, replace=False) for c in cnt])
        src = np.take_along_axis(rec, pick[..., None], axis=1)
        size = (src[..., 4:6] * (0.7 + 0.6 * rng.random(src[..., 4:6].shape))).astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        loader.append(Batch(img, t(rng.random(pick.shape) < 0.9), t(src[..., 0].astype(np.int64)), t(src[..., 2:4]),
                            t(size)))
        scores.append(rec[..., 1].reshape(-1))
    thr = np.quantile(np.concatenate(scores), np.linspace(0.0, 0.95, 10)).astype(np.float32)
    return loader, torch.from_numpy(thr)


def ten_pass(model, mc, loader, thr):
    """evaluate.py:211-233 / :167-208 on this package's API, the matching on the host."""
    precision, recall = [], []
    for t in thr.tolist():
        n_tp = n_det = n_truth = 0
        for batch in loader:
            with torch.no_grad():
                dets = tv.decode(model.forward(batch.img), mc, 100, t)
            rec, cnt = eval_ref.records_from_detections(dets)
            _, a, b, c = eval_ref.evaluate(rec, cnt, eval_ref.DECODE_COLUMNS, batch.valid.cpu().numpy(),
                                           batch.label.cpu().numpy(), batch.center.cpu().numpy(),
                                           batch.size.cpu().numpy(), eval_ref.BOX, IOU, [0.0])
            n_tp, n_det, n_truth = n_tp + int(a[0]), n_det + int(b[0]), n_truth + c
        p, r = eval_ref.precision_recall(n_tp, n_det, n_truth)
        precision.append(p)
        recall.append(r)
    return precision, recall


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launches(model, mc, loader, thr, dev):
    """Kernel launches of one batch of the one-pass path by kind, and the device-to-host copies of a whole
    curve, from a profiler trace. Raises where the profiler gives no device events: the two structural
    claims are asserted by main(), never assumed."""
    from torch.profiler import ProfilerActivity, profile

    def trace(batches):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            tv.evaluate_precision_recall_curve(model, mc, batches, dev, IOU, score_thresholds=thr)
            torch.cuda.synchronize()
        return [e for e in prof.events() if str(e.device_type).endswith("CUDA")]

    one, two, whole = trace(loader[:1]), trace(loader[:2]), trace(loader)
    if not one or not two or not whole:
        raise RuntimeError("the profiler recorded no device events: the launch counts cannot be checked")
    is_copy = lambda n: "memcpy" in n.lower() or "copy" in n.lower() and "kernel" not in n.lower()
    is_fill = lambda n: "memset" in n.lower() or "fillbuffer" in n.lower()
    kernels = lambda ev: [e.name for e in ev if not is_copy(e.name) and not is_fill(e.name)]
    per_batch = kernels(two)[len(kernels(one)):]  # the second batch: no buffer set-up
    evaluate = [n for n in per_batch if "evaluate" in n]
    squeeze = lambda n: n.lower().replace(" ", "").replace("_", "").replace("-", "")
    d2h = [e.name for e in whole if is_copy(e.name) and ("dtoh" in squeeze(e.name) or "devicetohost" in squeeze(e.name))]
    return dict(kernels_per_batch=len(per_batch), evaluate_kernels_per_batch=len(evaluate),
                kernel_names_per_batch=per_batch, evaluate_kernels_whole_curve=len([n for n in kernels(whole)
                                                                                    if "evaluate" in n]),
                device_to_host_copies_per_data_set=len(d2h),
                copy_event_names=sorted(set(e.name for e in whole if is_copy(e.name))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds: ten_pass once, one_pass --inner times")
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "eval_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    model, mc = build(dev)
    loader, thr = make_loader(model, mc, dev)
    curve = lambda: tv.evaluate_precision_recall_curve(model, mc, loader, dev, IOU, score_thresholds=thr)
    curve()  # warm-up of both sides
    ten_pass(model, mc, loader[:1], thr[:1])
    one, ten = [], []
    for _ in range(args.rounds):  # alternated, every sample kept
        t, (p10, r10) = wall_s(lambda: ten_pass(model, mc, loader, thr))
        ten.append(t)
        for _ in range(args.inner):
            t, (p1, r1) = wall_s(curve)
            one.append(t)
    same = p1.tolist() == p10 and r1.tolist() == r10
    counts = launches(model, mc, loader, thr, dev)
    res = dict(workload=f"r18 c128 fp16 {IN_H}x{IN_W}, {BATCHES} batches of {B}, {N} truths per image, 10 thresholds",
               one_pass_s=float(np.median(one)), ten_pass_s=float(np.median(ten)),
               one_pass_samples_s=one, ten_pass_samples_s=ten, one_pass_min_max_s=[min(one), max(one)],
               ten_pass_min_max_s=[min(ten), max(ten)], speedup=float(np.median(ten) / np.median(one)),
               curves_equal=same, precision=p1.tolist(), recall=r1.tolist(), score_thresholds=thr.tolist(),
               launches=counts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    assert same, "the one-pass curve differs from the ten-pass curve"
    assert max(r1.tolist()) > 0 and len(set(p1.tolist())) > 1, "the workload matches nothing: the curves say nothing"
    assert counts["evaluate_kernels_per_batch"] == 1 and counts["evaluate_kernels_whole_curve"] == BATCHES, \
        "not one evaluation launch per batch"
    assert counts["device_to_host_copies_per_data_set"] == 1, "not one device-to-host copy per data set"


if __name__ == "__main__":
    main()
