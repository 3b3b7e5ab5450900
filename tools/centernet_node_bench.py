"""CenterNet node step: the captured CenternetDetector step + host() against the sequence of separate
calls it replaces, and the keypoint matching kernel alone.

Workload: CenterpointDLA34 (one label with five keypoints, seeded weights), 480 x 640 uint8 frames,
depth 360 x 640, fp16, K = 10 objects / 50 keypoints, at B = 1 and B = 64. A seeded model's scores are
low, so the thresholds are 0.05: the counts reach K and K_kp and every keypoint has candidates (the
counts and the number of matches are in the output). Five keypoints per object keep the host PnP (six
or more matches, OpenCV) out of both sides.

  baseline  model.forward_frames -> decode_keypoints (host matching) -> localize_detections, wall time
            per step, frames and depth already on the device;
  new       one replay of the graph captured around CenternetDetector(frames, ..., depth, camera), then
            host(): wall time per step, same inputs, same process.
Both are run in three alternating rounds of `--steps` steps after `--warmup`; a round's figure is its
median, a side's the median of its three rounds, and `baseline_spread_ms` is max - min of the
baseline's three. `b1_ok` says whether the new step at B = 1 is no slower than the baseline beyond
that spread.

  kernel    tv_match_keypoints alone (DeviceKeypointDecoder.match) on the planted scenes of
            tests/keypoint_match_ref.py at B = 1 and B = 64: K = 10 / K_kp = 50 (the LDS-table route) and
            K = 70 / K_kp = 130 (errors computed inside the walk); HIP-event time of a replayed graph of
            `--inner` launches, median over `--repeats` replays (tools/localize_bench.py's scheme).
Prints one line per figure and a final JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import keypoint_match_ref as ref  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402
from localize_bench import graph_us  # noqa: E402
from recipe import seeded_u8_frames  # noqa: E402

IN_H, IN_W, DH, DW = 480, 640, 360, 640
K, K_KP, THR, KP_THR = 10, 50, 0.05, 0.05
M = np.array([[554.0 / 2 * 1.33, 0.0, 320.0 / 2], [0.0, 554.0 / 2 * 1.33, 180.0 / 2], [0.0, 0.0, 1.0]])
CAM = (float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2]))


def build_model(dev):
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig("o0", A(False, 1.0), A(False, 1.0), A(False, 1.0), True, True,
                                             [(0.1 * s, 0.0, 0.0) for s in range(5)])])
    model = tv.CenterpointDLA34(oc, precision="fp16").to(dev).eval()
    return model, oc, tv.ModelConfig([], [], IN_H, IN_W, 2, 1.0)


def wall_ms(step, steps, warmup):
    for _ in range(warmup):
        step()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def node_case(model, oc, mc, B, dev, steps, warmup):
    frames = seeded_u8_frames(B, IN_H, IN_W, seed=21).to(dev)
    rng = np.random.default_rng(3)
    depth_np = rng.integers(500, 6001, size=(B, DH, DW)).astype(np.uint16)
    depth_np[rng.random((B, DH, DW)) < 0.1] = 0
    depth = torch.from_numpy(depth_np).to(dev)

    def baseline():
        pred = model.forward_frames(frames, (IN_H, IN_W))
        dets = tv.decode_keypoints(pred, mc, oc, M, K, K_KP, THR, KP_THR, 0.0)
        return dets, tv.localize_detections(dets, depth, M)

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        det = tv.CenternetDetector(model, B, (IN_H, IN_W), mc, K, K_KP, dev)
        det(frames, THR, KP_THR, depth, CAM)  # the eager step on the capture stream
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        det(frames, THR, KP_THR, depth, CAM)

    def new():
        graph.replay()
        return det.host()

    # the two sides see the same detections
    dets, points = baseline()
    host = new()
    assert [len(d) for d in dets] == host.counts.tolist()
    n_match = sum(k is not None for im in dets for d in im for k in d.keypoints)
    valid = sum(p is not None for im in points for p in im)
    assert valid == int(host.points[..., 3].sum())
    rounds = {"baseline": [], "new": []}
    for _ in range(3):
        rounds["baseline"].append(wall_ms(baseline, steps, warmup))
        rounds["new"].append(wall_ms(new, steps, warmup))
    base, newm = float(np.median(rounds["baseline"])), float(np.median(rounds["new"]))
    return dict(B=B, steps=steps, warmup=warmup, baseline_ms=base, new_ms=newm,
                baseline_rounds_ms=rounds["baseline"], new_rounds_ms=rounds["new"],
                baseline_spread_ms=max(rounds["baseline"]) - min(rounds["baseline"]), ratio=base / newm,
                counts=host.counts.tolist()[:4], keypoint_counts=host.keypoint_counts.tolist()[:4],
                matched_host=n_match, matched_device=int(host.n_matched.sum()), valid_points=valid)


def kernel_case(name, B, dev, inner, repeats):
    scene = ref.make_scene(name, 1, B=B)
    from tauv_vision_amd.centernet import Prediction
    fields = {f: None for f in Prediction.__dataclass_fields__}
    for f in ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size", "offset", "depth"):
        fields[f] = getattr(scene.pred, f).to(dev)
    dec = tv.DeviceKeypointDecoder(B, len(scene.slots), len(scene.owner), scene.H, scene.W, scene.K, scene.K_kp,
                                   ref.object_config(scene), dev)
    dec(Prediction(**fields), tv.ModelConfig([], [], 4 * scene.H, 4 * scene.W, 2, 1.0), 0.2, scene.kp_thr)
    host = dec.host()
    us = graph_us(dec.match, dev, inner, repeats)
    return dict(scene=name, B=B, K=scene.K, K_kp=scene.K_kp, route="table" if scene.K * scene.K_kp <= 4096 else "walk",
                us=us, mean_objects=float(host.counts.float().mean()), mean_keypoints=float(host.keypoint_counts.float().mean()),
                matched=int(host.n_matched.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--steps-b64", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="launches per replayed graph (kernel timing)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node", "centernet_node_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kernel = []
    for name in ("A", "B"):
        for B in (1, 64):
            r = kernel_case(name, B, dev, args.inner, args.repeats)
            kernel.append(r)
            print(f"match kernel scene {name} ({r['route']:5s}) B={B:2d} K={r['K']:2d}/{r['K_kp']:3d}: {r['us']:8.1f} us, "
                  f"{r['mean_objects']:.1f} objects, {r['mean_keypoints']:.1f} keypoints per image, {r['matched']} matched",
                  flush=True)
    model, oc, mc = build_model(dev)
    node = []
    for B, steps in ((1, args.steps), (64, args.steps_b64)):
        r = node_case(model, oc, mc, B, dev, steps, args.warmup)
        node.append(r)
        print(f"node step B={B:2d}: baseline {r['baseline_ms']:8.3f} ms (spread {r['baseline_spread_ms']:.3f}), new "
              f"{r['new_ms']:8.3f} ms, ratio {r['ratio']:.2f}; counts {r['counts']} / {r['keypoint_counts']}, matched "
              f"{r['matched_device']} (host {r['matched_host']}), valid points {r['valid_points']}", flush=True)
    b1 = node[0]
    line = json.dumps(dict(tool="centernet_node_bench", model="CenterpointDLA34 fp16", frames=[IN_H, IN_W], depth=[DH, DW],
                           K=K, K_kp=K_KP, thresholds=[THR, KP_THR], node=node, kernel=kernel,
                           b1_ok=b1["new_ms"] <= b1["baseline_ms"] + b1["baseline_spread_ms"]))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
