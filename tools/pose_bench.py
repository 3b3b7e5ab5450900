"""The pose stage: what tv_solve_poses costs, alone and inside the CenterNet detector.

  kernel    tv_solve_poses alone on hand-made records, every detection valid with 8 keypoints at 0.5 px
            noise, K = 10, at B = 1 and B = 64, for the reference's 8-point model and for the planar
            octagon: the HIP-event time of a replayed graph of `--inner` calls, median over `--repeats`
            replays (tools/localize_bench.py's scheme). One launch of B * K one-wave workgroups; at B = 1 the
            time is the longest detection's chain (linear start, then the LM iterations), not throughput.
  host      the comparator: tests/pnp_ref.py (numpy float64, NOT OpenCV, which this stack does not have and
            cannot be measured here) solving the same records on the host, wall time per batch.
  detector  CenternetDetector on tools/centernet_node_bench.py's model and shapes (CenterpointDLA34 fp16,
            480 x 640, B = 1, K = 10, K_kp = 50) with an 8-keypoint object, captured in one graph: wall time
            per call (replay + host()) without and with poses=True. Seeded weights match few keypoints, so
            this prices the launch and the larger packed copy; the kernel cases price the solve.
The tool fails unless every pose meets the bar of tests/test_gpu_poses.py against pnp_ref and the detector's
host() makes one device-to-host copy per call. Prints one line per case and a final JSON line, also written
to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pnp_ref as P  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402
from centernet_node_bench import IN_H, IN_W, K, K_KP, KP_THR, THR, CAM as NODE_CAM, wall_ms  # noqa: E402
from localize_bench import graph_us  # noqa: E402
from recipe import seeded_u8_frames  # noqa: E402

MODELS, M_PROJ, (FRAME_H, FRAME_W) = P.load_models()
CAM = (M_PROJ[0, 0], M_PROJ[1, 1], M_PROJ[0, 2], M_PROJ[1, 2])


def kernel_case(name, B, dev, inner, repeats):
    planar = name == "octagon"
    obj = P.octagon() if planar else MODELS[name]
    A = tv.AngleConfig(False, None)
    oc = tv.ObjectConfigSet([tv.ObjectConfig("o", A, A, A, False, True, [tuple(float(v) for v in p) for p in obj])])
    table = tv.pose_model_points(oc)
    rng = np.random.default_rng(7 + B)
    dets, truths = [], {}
    for b in range(B):
        objs = []
        for d in range(K):
            R, t = P.tilted_pose(rng) if planar else P.random_pose(rng)
            uv, _ = P.project(R, t, obj, CAM)
            uv = uv + rng.normal(scale=0.5, size=uv.shape)
            objs.append((0, {s: tuple(uv[s]) for s in range(8)}))
            truths[(b, d)] = (R, t)
        dets.append(objs)
    arrays = P.make_records(dets, K, 8 * K, 8, FRAME_H, FRAME_W)
    rec, cnt, kp, kcnt, slot = (torch.from_numpy(a).to(dev) for a in arrays)
    solver = tv.DevicePoseSolver(B, K, 8 * K, oc, dev)
    mc = tv.ModelConfig([], [], FRAME_H, FRAME_W, 2, 1.0)
    run = lambda: solver(rec, cnt, kp, kcnt, slot, mc, CAM)
    got = run().cpu().numpy()
    t0 = time.perf_counter()
    ref, bars = P.reference_and_bars(arrays, table, FRAME_H, FRAME_W, CAM, truths)
    both_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    P.solve_poses(*arrays, table, FRAME_H, FRAME_W, CAM)
    host_ms = (time.perf_counter() - t0) * 1e3
    worst = P.assert_poses(got, ref, bars, f"{name} B={B}")
    assert int(ref[..., 12].sum()) == B * K, "not every detection is valid"
    return dict(model=name, B=B, K=K, solve_us=graph_us(run, dev, inner, repeats), host_pnp_ref_ms=host_ms,
                max_iterations=int(got[..., 15].max()), mean_iterations=float(got[..., 15].mean()),
                worst_angle=float(worst[0]), worst_dt=float(worst[1]), worst_rms=float(worst[2]),
                largest_bar=float(bars.max()), reference_and_spread_ms=both_ms)


def detector_case(dev, steps, warmup):
    A = tv.AngleConfig(False, 1.0)
    oc = tv.ObjectConfigSet([tv.ObjectConfig("o0", A, A, A, True, True, [tuple(float(v) for v in p) for p in MODELS["eight"]])])
    model = tv.CenterpointDLA34(oc, precision="fp16").to(dev).eval()
    mc = tv.ModelConfig([], [], IN_H, IN_W, 2, 1.0)
    frames = seeded_u8_frames(1, IN_H, IN_W, seed=21).to(dev)
    out = {}
    for poses in (False, True):
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            det = tv.CenternetDetector(model, 1, (IN_H, IN_W), mc, K, K_KP, dev, poses=poses)
            call = (lambda: det(frames, THR, KP_THR, None, NODE_CAM)) if poses else (lambda: det(frames, THR, KP_THR))
            call()
            s.synchronize()
        torch.cuda.current_stream(dev).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()

        def step():
            graph.replay()
            return det.host()

        copies, real = [], torch.Tensor.copy_

        def counting(self, src, *a, **k):
            if isinstance(src, torch.Tensor) and src.is_cuda and not self.is_cuda:
                copies.append(src.numel())
            return real(self, src, *a, **k)

        torch.Tensor.copy_ = counting
        try:
            host = step()
        finally:
            torch.Tensor.copy_ = real
        assert len(copies) == 1, f"host() made {len(copies)} device-to-host copies"
        rounds = [wall_ms(step, steps, warmup) for _ in range(3)]
        key = "with_poses" if poses else "without"
        out[key + "_ms"] = float(np.median(rounds))
        out[key + "_rounds_ms"] = rounds
        out[key + "_copy_bytes"] = copies[0]
        out[key + "_graph_us"] = graph_us(call, dev, 5, 9)
        if poses:
            out["valid_poses"] = int(host.poses[..., 12].sum())
            out["matched"] = int(host.n_matched.sum())
    out["added_ms"] = out["with_poses_ms"] - out["without_ms"]
    out["added_graph_us"] = out["with_poses_graph_us"] - out["without_graph_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="calls per replayed graph")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose", "pose_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = []
    for name in ("eight", "octagon"):
        for B in (1, 64):
            r = kernel_case(name, B, dev, args.inner, args.repeats)
            cases.append(r)
            print(f"{name:8s} B={B:2d}: tv_solve_poses {r['solve_us']:8.1f} us per call ({B * K} poses, at most "
                  f"{r['max_iterations']} LM iterations), pnp_ref on the host {r['host_pnp_ref_ms']:.1f} ms; worst angle "
                  f"{r['worst_angle']:.2e}, |dt|/|t| {r['worst_dt']:.2e}, bar {r['largest_bar']:.2e}", flush=True)
    det = detector_case(dev, args.steps, args.warmup)
    print(f"detector B=1: {det['without_ms']:.3f} ms per call, {det['with_poses_ms']:.3f} ms with poses "
          f"(+{det['added_ms'] * 1e3:.1f} us wall, +{det['added_graph_us']:.1f} us in the graph; {det['matched']} keypoints "
          f"matched, {det['valid_poses']} poses valid)", flush=True)
    line = json.dumps(dict(tool="pose_bench", comparator="pnp_ref (numpy float64), not OpenCV", inner=args.inner,
                           repeats=args.repeats, kernel=cases, detector=det))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
