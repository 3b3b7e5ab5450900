"""YOLACT evaluation timing probe: box and mask average precision on the device (csrc/yolact_eval.hip,
tauv_vision_amd/yolact_evaluate.py) on the reference's 640 x 360 training config (yolact/scripts/
train.py:28-49: the production head on the ResNet-18 backbone), seeded weights with the classification
layer scaled by 1 / 64 so that the confidences are graded, fp16, top_k = 100, at B = 8 and 24. The data
set is --batches batches of seeded images already on the device; 8 truths per image are planted from the
model's own detections (every other one: its box, its label and its frame-size mask painted into the seg
map in descending score), so the matching has work and the masks overlap the truths.

Measured per B:
  * HIP-event time of a replayed graph, median of --repeats: the two new C-ABI calls alone
    (DeviceYolactEvaluator.update: four launches), and the whole step of one batch — the detector call
    with frame_masks="bilinear" plus the detection_records call for the softmax rows — with and without
    them;
  * wall time of the whole data set by tv.evaluate_average_precision;
  * wall time of the same answer the way a user gets it today on this package: the same detector and
    records calls, unpack_frame_masks, per image the [K, H, W] x [N, H, W] overlap in torch on the device,
    the copy to the host, and the host matching and AP of tests/yolact_eval_ref.py.
The tool FAILS unless the two evaluations are equal, one batch launches exactly four kernels of the new
file (zeroing, overlap, matching, cursor) and a data set makes exactly one device-to-host copy — counted
from a torch.profiler trace, never assumed — or if the profiler gives no device events. No time is a
condition. Prints a JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tauv_vision_amd as tv  # noqa: E402
import yolact_eval_ref as ref  # noqa: E402
from tauv_vision_amd.yolact import unpack_frame_masks  # noqa: E402

IN_H, IN_W, TOP_K, N_TRUTH, NMS_IOU, CONFIDENCE = 360, 640, 100, 8, 0.5, 0.05
LAUNCHES_PER_BATCH = 4  # zeroing + overlap, matching + cursor step


def build():
    import resnet18_ref as rr
    from recipe_yolact_head import SCALES, VAR, head_case, head_inputs
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact, YolactConfig
    c = dict(head_case("yolact_head_d"), in_h=IN_H, in_w=IN_W)
    head_sd, _ = head_inputs(c)
    full = {"_backbone._feature_extractor." + k: v for k, v in rr.seeded_resnet18_state_dict(0).items()}
    full.update(head_sd)
    for k in ("_prediction_head._classification_layer.weight", "_prediction_head._classification_layer.bias"):
        full[k] = full[k] / 64
    cfg = YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])
    net = Yolact(cfg, backbone=Resnet101Backbone(cfg, "fp16"), precision="fp16")
    net.load_state_dict(full, strict=True)
    return net


class Step:
    """One batch's device work: the detector, the records call for the softmax rows, and (optionally) update."""

    def __init__(self, net, B, dev):
        self.det = tv.YolactDetector(net, B, (IN_H, IN_W), TOP_K, dev, frame_masks="bilinear")
        self.conf = torch.zeros((B, self.det.K, self.det.head_out[0].shape[2]), dtype=torch.float32, device=dev)

    def detect(self, img):
        d = self.det
        res = d(img, NMS_IOU, CONFIDENCE)
        tv.detection_records(d.head_out[0], d.box, d.det, d.counts, out=d.records, confidence_out=self.conf)
        return res


def label_score(conf):
    fg = conf[:, 1:]
    return 1 + fg.argmax(1), fg.max(1)


def make_loader(net, B, batches, dev):
    step = Step(net, B, dev)
    g = torch.Generator().manual_seed(7)
    loader = []
    for _ in range(batches):
        img = torch.randn((B, 3, IN_H, IN_W), generator=g).to(dev)
        res = step.detect(img)
        counts, conf, rec = res.counts.cpu().numpy(), step.conf.cpu().numpy(), res.records.cpu().numpy()
        seg = np.full((B, IN_H, IN_W), 255, dtype=np.uint8)
        valid = np.zeros((B, N_TRUTH), dtype=bool)
        label = np.zeros((B, N_TRUTH), dtype=np.int64)
        box = np.zeros((B, N_TRUTH, 4), dtype=np.float32)
        for b in range(B):
            c = int(counts[b])
            if c == 0:
                continue
            labels, scores = label_score(conf[b, :c])
            chosen = list(range(0, c, 2))[:N_TRUTH]
            masks = unpack_frame_masks(res.bits[b, :c], IN_W).cpu().numpy()
            for t, d in enumerate(chosen):
                valid[b, t], label[b, t], box[b, t] = True, labels[d], rec[b, d, 4:8]
            for d in sorted(chosen, key=lambda d: -float(scores[d])):
                seg[b][masks[d] & (seg[b] == 255)] = chosen.index(d)
        t = lambda a: torch.from_numpy(a).to(dev)
        loader.append(SimpleNamespace(img=img, seg=t(seg), valid=t(valid), classifications=t(label),
                                      bounding_boxes=t(box)))
    return loader


def today(net, loader, dev, step):
    """The same answer without the new kernels: torch on the device for the overlap, the host for the rest."""
    thr = ref.default_thresholds()
    logs, n_truth = [], 0
    for s in loader:
        res = step.detect(s.img)
        B, K = res.records.shape[:2]
        N = s.valid.shape[1]
        inter = torch.empty((B, K, N), device=dev)
        det_area = torch.empty((B, K), device=dev)
        truth_area = torch.empty((B, N), device=dev)
        ids = torch.arange(N, device=dev).view(N, 1, 1)
        for b in range(B):
            m = unpack_frame_masks(res.bits[b], IN_W)  # [K, H, W] bool
            m = m & (torch.arange(K, device=dev) < res.counts[b]).view(K, 1, 1)
            img_valid = s.seg[b] != 254
            truth = (s.seg[b].unsqueeze(0) == ids) & s.valid[b].view(N, 1, 1) & img_valid  # [N, H, W]
            mf = (m & img_valid).float()
            inter[b] = torch.einsum("khw,nhw->kn", mf, truth.float())  # (counts < 2^24: exact in fp32)
            det_area[b] = mf.sum((1, 2))
            truth_area[b] = truth.float().sum((1, 2))
        host = [t.cpu().numpy() for t in (inter, det_area, truth_area, res.counts, step.conf, res.records, s.valid,
                                          s.classifications, s.bounding_boxes)]
        i, da, ta, counts, conf, rec, valid, label, box = host
        for b in range(B):
            _, lg = ref.walk_image(conf[b], rec[b], counts[b], valid[b], label[b], box[b], i[b].astype(np.int64),
                                   da[b].astype(np.int64), ta[b].astype(np.int64), thr)
            logs.append(lg)
            for t in range(N):
                if valid[b, t]:
                    n_truth = n_truth + np.eye(conf.shape[2], dtype=np.int64)[int(label[b, t])]
    return tv.average_precision(np.stack(logs), n_truth, len(thr))


def graph_us(fn, dev, repeats):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(repeats + 2):
        ev[0].record()
        graph.replay()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return float(np.median(times[2:])), [float(t) for t in times[2:]]


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launches(net, loader, dev):
    """Kernels of the new file in one batch, and device-to-host copies of a whole data set, from a trace."""
    from torch.profiler import ProfilerActivity, profile

    def trace(batches):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            tv.evaluate_average_precision(net, batches, dev, TOP_K, NMS_IOU, CONFIDENCE)
            torch.cuda.synchronize()
        return [e for e in prof.events() if str(e.device_type).endswith("CUDA")]

    one, two, whole = trace(loader[:1]), trace(loader[:2]), trace(loader)
    if not one or not two or not whole:
        raise RuntimeError("the profiler recorded no device events: the launch counts cannot be checked")
    is_copy = lambda n: "memcpy" in n.lower() or "copy" in n.lower() and "kernel" not in n.lower()
    is_fill = lambda n: "memset" in n.lower() or "fillbuffer" in n.lower()
    kernels = lambda ev: [e.name for e in ev if not is_copy(e.name) and not is_fill(e.name)]
    per_batch = kernels(two)[len(kernels(one)):]
    count = lambda ev: len([n for n in kernels(ev) if "yeval" in n])
    new = [n for n in kernels(two) if "yeval" in n][count(one):]  # the second batch's
    squeeze = lambda n: n.lower().replace(" ", "").replace("_", "").replace("-", "")
    d2h = [e.name for e in whole if is_copy(e.name) and ("dtoh" in squeeze(e.name) or "devicetohost" in squeeze(e.name))]
    return dict(kernels_per_batch=len(per_batch), new_kernels_per_batch=count(two) - count(one), new_kernel_names=new,
                new_kernels_whole_data_set=count(whole),
                device_to_host_copies_per_data_set=len(d2h),
                copy_event_names=sorted(set(e.name for e in whole if is_copy(e.name))))


def case(net, B, dev, args):
    loader = make_loader(net, B, args.batches, dev)
    s0 = loader[0]
    step = Step(net, B, dev)
    C = step.conf.shape[2] - 1
    ev = tv.DeviceYolactEvaluator(B, step.det.K, N_TRUTH, C, (IN_H, IN_W), dev)
    ev.reserve(B * (args.repeats + 8) * 2)
    res = step.detect(s0.img)
    truths = (s0.seg, s0.valid, s0.classifications, s0.bounding_boxes)
    update = lambda: ev.update(res.bits, res.counts, step.conf, step.det.records, *truths)
    out = dict(B=B, batches=args.batches, K=step.det.K, n_classes=C, counts_first_batch=res.counts.cpu().tolist())
    out["update_us"], out["update_samples_us"] = graph_us(update, dev, args.repeats)
    ev.reset()
    out["step_without_us"], out["step_without_samples_us"] = graph_us(lambda: step.detect(s0.img), dev, args.repeats)
    out["step_with_us"], out["step_with_samples_us"] = graph_us(lambda: (step.detect(s0.img), update()), dev,
                                                               args.repeats)
    run = lambda: tv.evaluate_average_precision(net, loader, dev, TOP_K, NMS_IOU, CONFIDENCE)
    run()  # warm-up of both sides
    today(net, loader[:1], dev, step)
    new_s, old_s = [], []
    for _ in range(args.rounds):
        t, old = wall_s(lambda: today(net, loader, dev, step))
        old_s.append(t)
        t, new = wall_s(run)
        new_s.append(t)
    out.update(evaluate_s=float(np.median(new_s)), evaluate_samples_s=new_s, today_s=float(np.median(old_s)),
               today_samples_s=old_s, equal=bool(np.array_equal(new.ap, old.ap, equal_nan=True)
                                                 and np.array_equal(new.map, old.map)
                                                 and new.n_detections == old.n_detections),
               map=new.map.tolist(), ap50=new.ap50.tolist(), ap75=new.ap75.tolist(), n_truth=new.n_truth.tolist(),
               n_detections=new.n_detections, launches=launches(net, loader, dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--sizes", default="8,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "yolact_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yolact_eval_bench needs the MI355X: no HIP device is visible")
    dev = torch.device("cuda", 0)
    net = build()
    results = []
    for B in (int(v) for v in args.sizes.split(",")):
        results.append(case(net, B, dev, args))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    res = dict(tool="yolact_eval_bench", workload=f"yolact r18 production head fp16 {IN_H}x{IN_W}, top_k {TOP_K}, "
               f"{N_TRUTH} truths per image planted from the model's own detections, seeded weights",
               repeats=args.repeats, rounds=args.rounds, results=results,
               not_measured=["a profiler trace of the two kernels", "more than one GPU", "a real trained checkpoint"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    for r in results:
        assert r["equal"], f"B = {r['B']}: the device evaluation differs from today's path"
        assert 0 < r["map"][0] < 1 and 0 < r["map"][1] < 1, "the workload says nothing: map is 0 or 1"
        n = r["launches"]
        assert n["new_kernels_per_batch"] == LAUNCHES_PER_BATCH and \
            n["new_kernels_whole_data_set"] == LAUNCHES_PER_BATCH * r["batches"], "not four new launches per batch"
        assert n["device_to_host_copies_per_data_set"] == 1, "not one device-to-host copy per data set"


if __name__ == "__main__":
    main()
