"""Frame-size mask timing probe: frame_masks (csrc/yolact_frame.hip) from the 640 x 360 model's own
prototype size (180 x 320) to frames of 360 x 640 and 720 x 1280, at the node shape (B = 1, n = 10) and
batched (B = 32, n = 100), bilinear and nearest, with and without the overlay, bounded by the boxes as
YolactDetector runs it. HIP-event time of a replayed graph of `--inner` calls, median over `--repeats`
replays. Bytes are computed from the shapes: every mask value once, the packed bits and areas written,
and with the overlay the frame read and the overlay written (bound_by_box reads fewer mask values:
the figure is an upper bound, and GB/s with it).

Beside it, what a user of model.detect() does today on the same inputs, in this tool's own words:
eager PyTorch-ROCm F.interpolate + `> 0.5` on the device per image, the [n, H, W] fp32 copy to the
host (yolact_node.py:135,143), and the numpy blend of utils/plot.py:148-152 per detection — timed with a
host clock around work that ends in a device synchronise, on the first `--host-images` images, scaled to B.

Last, YolactDetector per call on the 640 x 360 model with and without the frame_masks step (graph
replay, uint8 frames at the model size).
Prints one line per case and a final JSON line (also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import tauv_vision_amd as tv  # noqa: E402
from tauv_vision_amd.yolact import DeviceFrameMasks, TAB10  # noqa: E402

MH, MW = 180, 320


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


def inputs(B, n, dev, seed):
    """Masks as assemble_mask leaves them: a smooth blob (sigmoid of a bicubically enlarged random field)
    inside each detection's box crop, zero outside; boxes 0.1 - 0.4 of the frame."""
    g = torch.Generator(device=dev).manual_seed(seed)
    box = torch.cat([torch.rand((B, n, 2), generator=g, device=dev) * 0.8 + 0.1,
                     torch.rand((B, n, 2), generator=g, device=dev) * 0.3 + 0.1], dim=-1).contiguous()
    masks = torch.empty((B, n, MH, MW), device=dev)
    ys = torch.arange(MH, device=dev, dtype=torch.float32).view(1, MH, 1)
    xs = torch.arange(MW, device=dev, dtype=torch.float32).view(1, 1, MW)
    for b in range(B):  # (per image: the bicubic intermediate of a whole batch would be large)
        field = torch.randn((1, n, 6, 10), generator=g, device=dev) * 2.0
        m = torch.sigmoid(F.interpolate(field, (MH, MW), mode="bicubic", align_corners=False))[0]
        by, bx = (box[b, :, 0] * MH).view(n, 1, 1), (box[b, :, 1] * MW).view(n, 1, 1)
        bh, bw = (box[b, :, 2] * MH).view(n, 1, 1), (box[b, :, 3] * MW).view(n, 1, 1)
        masks[b] = m * ((xs >= bx - bw / 2) & (xs <= bx + bw / 2) & (ys >= by - bh / 2) & (ys <= by + bh / 2)).float()
    records = torch.zeros((B, n, 8), device=dev)
    records[..., 1] = torch.randint(0, 12, (B, n), generator=g, device=dev).float()
    records[..., 4:] = box
    det = torch.arange(n, device=dev).repeat(B, 1).contiguous()
    return masks, box, det, records


def eager_today(masks, records, frames, H, W, mode, images):
    """The path without frame_masks, per image: F.interpolate + > 0.5 on the device, the fp32 [n, H, W] copy
    to the host, the numpy blend per detection. -> (seconds per image: device step, copy, blend)."""
    pal = TAB10.numpy()
    t_dev = t_copy = t_blend = 0.0
    for b in range(images):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "bilinear":
            up = F.interpolate(masks[b].unsqueeze(0), (H, W), mode="bilinear").squeeze(0)
        else:
            up = F.interpolate(masks[b].unsqueeze(0), (H, W)).squeeze(0)
        sel = up > 0.5
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mask_np = up.detach().cpu().numpy()  # yolact_node.py:143
        t2 = time.perf_counter()
        if frames is not None:
            vis = frames[b].cpu().numpy().copy()
            cls = records[b, :, 1].cpu().numpy()
            for d in range(mask_np.shape[0]):
                colour = pal[min(int(cls[d]), len(pal) - 1)].astype(np.float64)
                m = mask_np[d] > 0.5
                vis[m] = 0.5 * colour + 0.5 * vis[m]
        t3 = time.perf_counter()
        t_dev, t_copy, t_blend = t_dev + t1 - t0, t_copy + t2 - t1, t_blend + t3 - t2
        del up, sel, mask_np
    return t_dev / images, t_copy / images, t_blend / images


def case(B, n, H, W, dev, args):
    masks, box, det, records = inputs(B, n, dev, seed=B * 1000 + n)
    counts = torch.full((B,), n, dtype=torch.int32, device=dev)
    frames = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator(device=dev).manual_seed(H), dtype=torch.uint8,
                           device=dev)
    step = DeviceFrameMasks(B, n, (H, W), dev)
    ww = (W + 31) // 32
    out = []
    for mode in ("bilinear", "nearest"):
        for overlay in (False, True):
            fr, rec = (frames, records) if overlay else (None, None)
            inner = args.inner if B * n * H * W < 5e7 else max(args.inner // 10, 1)  # (the large cases take milliseconds)
            us = graph_us(lambda: step(masks, counts, mode, det, box, fr, rec), dev, inner, args.repeats)
            nbytes = 4 * B * n * (MH * MW + H * ww + 1) + (2 * 3 * B * H * W if overlay else 0)
            hb = min(B, args.host_images)
            eager_today(masks, records, fr, H, W, mode, 1)  # warm-up
            t_dev, t_copy, t_blend = eager_today(masks, records, fr, H, W, mode, hb)
            out.append(dict(case=f"B={B} n={n} {H}x{W} {mode}" + (" overlay" if overlay else ""), B=B, n=n, H=H, W=W,
                            mode=mode, overlay=overlay, us=us, bytes=nbytes, gbps=nbytes / us * 1e-3,
                            area_share=float(step.area.double().mean()) / (H * W),
                            eager_interpolate_us=t_dev * 1e6 * B, eager_copy_us=t_copy * 1e6 * B,
                            eager_blend_us=t_blend * 1e6 * B, eager_us=(t_dev + t_copy + t_blend) * 1e6 * B,
                            eager_images_timed=hb))
    return out


def detector_case(B, top_k, dev, args):
    """YolactDetector per call on the 640 x 360 model (tests' seeded weights), with and without the step."""
    import resnet18_ref as rr
    from recipe import seeded_u8_frames
    from recipe_yolact_head import SCALES, VAR, head_case, head_inputs
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact, YolactConfig
    c = dict(head_case("yolact_head_d"), in_h=360, in_w=640)  # the production head at the node's 640 x 360
    head_sd, _ = head_inputs(c)
    full = {"_backbone._feature_extractor." + k: v for k, v in rr.seeded_resnet18_state_dict(0).items()}
    full.update(head_sd)
    cfg = YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])
    net = Yolact(cfg, backbone=Resnet101Backbone(cfg, "fp16"), precision="fp16")
    net.load_state_dict(full, strict=True)
    hw = (c["in_h"], c["in_w"])
    frames = seeded_u8_frames(B, hw[0], hw[1], seed=3).to(dev)
    res = dict(B=B, top_k=top_k, frame=list(hw))
    for mode in (None, "bilinear", "nearest"):
        detector = tv.YolactDetector(net, B, hw, top_k, dev, frame_masks=mode)
        res[f"us_{mode or 'without'}"] = graph_us(lambda: detector(frames, 0.5, 0.05), dev, max(args.inner // 4, 1),
                                                  args.repeats)
        res["counts"] = detector.counts.cpu().tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="calls per replayed graph")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-images", type=int, default=1, help="images the eager path is timed on")
    ap.add_argument("--shapes", default="1x10,32x100", help="BxN pairs")
    ap.add_argument("--frames", default="360x640,720x1280")
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_masks", "frame_masks_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yolact_frame_masks_bench needs the MI355X: no HIP device is visible")
    dev = torch.device("cuda", 0)
    results = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        for size in args.frames.split(","):
            H, W = (int(v) for v in size.split("x"))
            for r in case(B, n, H, W, dev, args):
                results.append(r)
                print(f"{r['case']:42s}: {r['us']:10.1f} us {r['bytes'] / 1e6:9.2f} MB {r['gbps']:8.1f} GB/s | eager "
                      f"{r['eager_us'] / 1e3:10.2f} ms (interpolate {r['eager_interpolate_us'] / 1e3:.2f}, copy "
                      f"{r['eager_copy_us'] / 1e3:.2f}, blend {r['eager_blend_us'] / 1e3:.2f})", flush=True)
            torch.cuda.empty_cache()
    detectors = []
    if not args.no_detector:
        for B, top_k in ((1, 10), (32, 100)):
            detectors.append(detector_case(B, top_k, dev, args))
            print("YolactDetector", json.dumps(detectors[-1]), flush=True)
    line = json.dumps(dict(tool="yolact_frame_masks_bench", mask=[MH, MW], inner=args.inner, repeats=args.repeats,
                           host_images=args.host_images, results=results, detector=detectors))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
