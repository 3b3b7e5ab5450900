"""Depth-localisation timing probe: DeviceLocalizer.boxes / .masks at the node shape (B = 1, depth
360 x 640, K = 10 boxes or n = 10 masks of 90 x 160) and at the batched shape (B = 64, K = 100).
HIP-event time of a replayed graph of `--inner` launches, median over `--repeats` replays; bytes
read are counted from the regions (2 B per depth pixel scanned, plus 4 B per mask value of each
scanned detection). The baseline is tests/localize_ref.py's host loop (the nodes' numpy / torch
code) on the same inputs, timed on the first `--host-images` images and scaled to B.
Prints one line per case and a final JSON line (also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import localize_ref as ref  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402

DH, DW, MH, MW, A = 360, 640, 90, 160, 200
M = np.array([[554.0 / 2 * 1.33, 0.0, 320.0 / 2], [0.0, 554.0 / 2 * 1.33, 180.0 / 2], [0.0, 0.0, 0.0]])
CAM = (float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2]))


def graph_us(fn, dev, inner, repeats):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for _ in range(inner):
            fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(repeats + 2):
        ev[0].record()
        graph.replay()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3 / inner)
    return float(np.median(times[2:]))


def clipped(lo, hi, n):
    lo, hi = max(min(lo, hi), 0), min(max(lo, hi), n - 1)
    return max(hi - lo + 1, 0)


def inputs(B, K, seed):
    rng = np.random.default_rng(seed)
    depth = rng.integers(500, 6001, size=(B, DH, DW)).astype(np.uint16)
    depth[rng.random((B, DH, DW)) < 0.1] = 0
    yx = rng.uniform(0.1, 0.9, size=(B, K, 2))
    hw = rng.uniform(0.1, 0.4, size=(B, K, 2))
    rec = np.zeros((B, K, 10), dtype=np.float32)
    rec[..., 2:4] = yx
    rec[..., 4:6] = hw
    return depth, rec


def box_pixels(rec):
    n = 0
    for y, x, h, w in rec[..., 2:6].reshape(-1, 4).astype(np.float64):
        ex, ey, W, H = x * DW, y * DH, w * DW, h * DH
        n += clipped(int(ex - 0.4 * W), int(ex + 0.4 * W), DW) * clipped(int(ey - 0.4 * H), int(ey + 0.4 * H), DH)
    return n


def case(name, B, K, dev, args):
    depth_np, rec_np = inputs(B, K, 1)
    depth = torch.from_numpy(depth_np).to(dev)
    rec = torch.from_numpy(rec_np).to(dev)
    counts = torch.full((B,), K, dtype=torch.int32, device=dev)
    loc = tv.DeviceLocalizer(B, K, dev)
    out = []
    # box mode
    us = graph_us(lambda: loc.boxes(rec, counts, depth, *CAM), dev, args.inner, args.repeats)
    nbytes = 2 * box_pixels(rec_np)
    hb = min(B, args.host_images)
    t0 = time.perf_counter()
    for b in range(hb):
        ref.centernet_localize([tuple(float(v) for v in r[2:6]) for r in rec_np[b]], depth_np[b], M)
    host_us = (time.perf_counter() - t0) * 1e6 * B / hb
    out.append(dict(case=f"{name} boxes", B=B, K=K, us=us, bytes=nbytes, gbps=nbytes / us * 1e-3, host_us=host_us))
    # mask mode: the boxes' own crops at mask resolution (0.9 inside, 0 outside), as assemble_mask leaves them
    box = torch.zeros((B, A, 4), device=dev)
    box[:, :K] = rec[..., 2:6]
    det = torch.arange(K, device=dev).repeat(B, 1)
    ys = torch.arange(MH, device=dev, dtype=torch.float32).view(1, 1, MH, 1)
    xs = torch.arange(MW, device=dev, dtype=torch.float32).view(1, 1, 1, MW)
    by, bx = (rec[..., 2] * MH).view(B, K, 1, 1), (rec[..., 3] * MW).view(B, K, 1, 1)
    bh, bw = (rec[..., 4] * MH).view(B, K, 1, 1), (rec[..., 5] * MW).view(B, K, 1, 1)
    masks = ((xs >= bx - bw / 2) & (xs <= bx + bw / 2) & (ys >= by - bh / 2) & (ys <= by + bh / 2)).float() * 0.9
    masks = masks.contiguous()
    full_bytes = B * K * (2 * DH * DW + 4 * MH * MW)
    t0 = time.perf_counter()
    for b in range(hb):
        m = masks[b].cpu()  # the node copies the up-sampled [n, H, W] masks instead: the baseline is flattered
        ref.yolact_localize(m, list(range(K)), box[b].cpu(), depth_np[b], *CAM)
    host_us = (time.perf_counter() - t0) * 1e6 * B / hb
    for bound in (False, True):
        us = graph_us(lambda: loc.masks(masks, counts, det, box, depth, *CAM, bound_by_box=bound), dev, args.inner,
                      args.repeats)
        # bound_by_box: the crop is the box itself (w x h of the image) against box mode's 0.8 w x 0.8 h
        nbytes = full_bytes if not bound else int(sum(
            (2 * DH * DW + 4 * MH * MW) * min(float(r[4]), 1.0) * min(float(r[5]), 1.0)
            for r in rec_np.reshape(-1, 10)))
        out.append(dict(case=f"{name} masks" + (" bound_by_box" if bound else ""), B=B, K=K, us=us, bytes=nbytes,
                        gbps=nbytes / us * 1e-3, host_us=host_us, bytes_approx=bound))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="launches per replayed graph")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-images", type=int, default=1, help="images the host baseline is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    for name, B, K in (("node", 1, 10), ("batched", 64, 100)):
        for r in case(name, B, K, dev, args):
            results.append(r)
            print(f"{r['case']:28s} B={r['B']:3d} K={r['K']:3d}: {r['us']:9.1f} us  {r['bytes'] / 1e6:9.2f} MB "
                  f"{r['gbps']:8.1f} GB/s   host loop {r['host_us'] / 1e3:10.1f} ms", flush=True)
    line = json.dumps(dict(tool="localize_bench", depth=[DH, DW], mask=[MH, MW], inner=args.inner,
                           repeats=args.repeats, host_images=args.host_images, results=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
