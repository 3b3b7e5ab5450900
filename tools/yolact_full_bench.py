"""Time the whole YOLACT forward from the image at the benchmark geometry (550 x 550; ResNet-18 taps
128 x 69 x 69, 256 x 35 x 35, 512 x 18 x 18; F = 256, 7 classes, 8 prototypes, one aspect ratio, one
trunk block, two extra levels), batch 32 and batch 1:

  fused     Yolact(cfg, backbone=Resnet101Backbone(cfg)) — one native plan (TV_ARCH_YOLACT) — with
            caller-owned outputs, as a replayed graph;
  two_call  the native backbone, then YolactHead on its fp32 taps, as two eager calls (what the
            library offered per part: the taps leave the arena, are transposed and rounded again);
  torch     the same step in eager PyTorch-ROCm: tests/resnet18_ref.py + tests/yolact_head_ref.py with
            the weights and the image cast to the same dtype;
  knob A/B  the fused plan built through tv_engine_create_diag with each of --knobs (e.g. TV_RSTEM=0)
            against the default, alternating on the same box; a knob the library does not know is
            reported as such;
  frames    Yolact.forward_frames on uint8 NHWC camera frames at the model size (ToTensor + Normalize in
            the stem kernel's LUT), caller-owned outputs, as a replayed graph;
  torch_prep_then_fused  what a caller did before forward_frames existed: the torch-op ToTensor +
            Normalize of the same u8 frames into the fp32 NCHW image (eager), then the `fused` graph.

Each is timed with device events around `--steps` iterations after `--warmup` (a synchronise ends each
window), `--repeats` times, the variants alternating, on seeded inputs resident on the device: min /
median / max over the repeats. In separate passes: the per-op profile of the fused step (one op per
launch) summed per part — stem + pool, layer1..4, FPN, protonet, heads — against the same part in
PyTorch, so that a native part slower than its PyTorch counterpart is named (`slower_than_torch`), and the
stem + pool row of the same profile over the u8 frames next to the fp32 one (`stem_pool_ms`).
Prints one JSON line per batch and writes everything to --out.

Usage: python tools/yolact_full_bench.py [--batches 32,1] [--precision fp16] [--steps 100] [--warmup 10]
                                         [--repeats 3] [--knobs TV_RSTEM=0] [--out profiles/yolact_full/bench.json]
                                         [--lib tauv-vision_amd/lib_x/libtauv_vision_amd.so]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tauv-vision_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BB = "_backbone._feature_extractor."


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def graphed(net, img, dev, fwd=None):
    """One eager step on the capture stream (workspaces, anchors), then the captured `out=` step. `fwd`:
    the entry (net.forward_frames for uint8 frames; default the fp32 forward)."""
    fwd = fwd or net
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        first = fwd(img)
        out = [torch.empty_like(first[0]), torch.empty_like(first[1]), torch.empty_like(first[2]),
               torch.empty((img.shape[0],) + tuple(first[4].shape[2:]) + ((first[4].shape[1] + 3) // 4 * 4,), device=dev)]
        fwd(img, out=out)
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fwd(img, out=out)
    return graph, out


def part_of(label):
    if label.startswith("input staging") or label.startswith(BB + "conv1") or label.startswith(BB + "maxpool"):
        return "stem + pool"
    for L in range(1, 5):
        if label.startswith(f"{BB}layer{L}."):
            return f"layer{L}"
    if label.startswith("_feature_pyramid.") or label.startswith("pyramid "):
        return "fpn"
    if label.startswith("_masknet."):
        return "protonet"
    return "heads"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--knobs", default="TV_RSTEM=0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolact_full", "bench.json"))
    ap.add_argument("--lib", default="", help="another build of the library (an experiment build: make BUILD=... LIBDIR=... EXTRA=...)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yolact_full_bench needs the MI355X: no HIP device is visible")

    import resnet18_ref as rr
    import yolact_head_ref as yr
    from recipe_yolact_head import SCALES, VAR, head_case, head_inputs
    from tauv_vision_amd import _lib, engine as tv_engine
    from tauv_vision_amd.weights import geometry
    if a.lib:
        _lib.set_library_path(os.path.abspath(a.lib))
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact, YolactConfig, YolactHead

    c = head_case("yolact_head_d")
    head_sd, _ = head_inputs(c)
    bb_sd = rr.seeded_resnet18_state_dict(0)
    full = {BB + k: v for k, v in bb_sd.items()}
    full.update(head_sd)
    dev = torch.device("cuda", 0)
    cfg = YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(a.precision, torch.float32)

    def make(knobs=None):
        tv_engine.set_diagnostic_knobs(knobs)
        net = Yolact(cfg, backbone=Resnet101Backbone(cfg, a.precision), precision=a.precision)
        net.load_state_dict(full, strict=True)
        return net

    ref = rr.resnet18_ref(bb_sd, dt).to(dev)
    hsd = {k: v.to(dev, dt) if v.dtype.is_floating_point else v.to(dev) for k, v in head_sd.items()}
    results = []
    for B in [int(b) for b in a.batches.split(",")]:
        img = torch.randn((B, 3, c["in_h"], c["in_w"]), generator=torch.Generator(device=dev).manual_seed(2200), device=dev)
        imgd = img.to(dt)
        net = make()
        graph, out = graphed(net, img, dev)
        eng = next(iter(net._engines.values()))
        bb = net._backbone
        head = YolactHead((128, 256, 512), cfg, precision=a.precision)
        head.load_state_dict(head_sd, strict=True)
        taps = bb(img)
        hout = list(out)
        head(taps, out=hout)
        tout = [torch.empty_like(t) for t in bb.forward_nhwc(img)]

        def two_call():
            head(bb(img, out=tout), out=hout)

        def torch_step():
            with torch.no_grad():
                return yr.yolact_head(hsd, list(ref(imgd)), c["C"], c["k"])

        # from the camera's bytes: the u8 entry as a replayed graph, and the torch-op normalisation of the same
        # frames into a resident fp32 image followed by the fused graph over that image
        frames = torch.randint(0, 256, (B, c["in_h"], c["in_w"], 3), generator=torch.Generator(device=dev).manual_seed(2201),
                               dtype=torch.uint8, device=dev)
        fgraph, fout = graphed(net, frames, dev, net.forward_frames)
        mean = torch.tensor(cfg.img_mean, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(cfg.img_stddev, device=dev).view(1, 3, 1, 1)
        pimg = torch.empty_like(img)
        pgraph, pout = graphed(net, pimg, dev)

        def prep_then_fused():
            pimg.copy_((frames.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
            pgraph.replay()

        prep_then_fused()
        fgraph.replay()
        torch.cuda.synchronize()
        frames_equal = all(bool(torch.equal(x, y)) for x, y in zip(fout, pout))
        variants = {"fused_graph_ms": graph.replay, "two_call_eager_ms": two_call, "torch_eager_ms": torch_step,
                    "frames_graph_ms": fgraph.replay, "torch_prep_then_fused_graph_ms": prep_then_fused}
        # the knob A/B: the same plan built with each override, as replayed graphs on this box
        knob_note = {}
        for kv in [k for k in a.knobs.split(",") if k]:
            name, val = kv.split("=")
            try:
                knet = make({name: val})
                kgraph, kout = graphed(knet, img, dev)
                variants[f"fused_graph_{kv}_ms"] = kgraph.replay
                knob_note[kv] = {"max_abs_diff_vs_default": max(float((x - y).abs().max()) for x, y in zip(kout, out))}
            except ValueError as e:
                knob_note[kv] = {"not_run": str(e)}
        tv_engine.set_diagnostic_knobs(None)
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):  # alternating: a drift of the box hits every variant alike
            for k, fn in variants.items():
                runs[k].append(timed(fn, a.steps, a.warmup))
        tref = torch_step()
        graph.replay()
        torch.cuda.synchronize()
        # (a loose sanity figure, both being low precision: |native - torch|max over |torch|max per output)
        err = {n: round(float((x.float() - y.float()).abs().max()) / max(1.0, float(y.float().abs().max())), 6) for n, x, y in
               (("cls", out[0], tref[0]), ("enc", out[1], tref[1]), ("coef", out[2], tref[2]),
                ("proto", out[3][..., :c["k"]].permute(0, 3, 1, 2), tref[3]))}

        # per part: the fused plan's profile rows (one op per launch) against the part in PyTorch
        eng.profile_multi([img], out)
        rows = min((eng.profile_multi([img], out) for _ in range(3)), key=lambda r: sum(x[1] for x in r))
        native = {}
        for r in rows:
            native[part_of(r[0])] = native.get(part_of(r[0]), 0.0) + r[1]
        # the stem alone from either input kind: the stem + pool rows of alternating one-op-per-launch profiles
        stem = {"fp32": [], "u8": []}
        for _ in range(5):
            for kind, prof in (("fp32", lambda: eng.profile_multi([img], out)), ("u8", lambda: eng.profile_multi_u8(frames, fout))):
                stem[kind].append(sum(r[1] for r in prof() if part_of(r[0]) == "stem + pool"))
        u8_rows = eng.profile_multi_u8(frames, fout)
        stem_kernel = {"fp32": [r[3] for r in rows if r[0].startswith(BB + "maxpool")],
                       "u8": [r[3] for r in u8_rows if r[0].startswith(BB + "maxpool")]}
        psteps, pwarm = max(10, a.steps // 3), 3
        with torch.no_grad():
            x0 = ref.maxpool(F.relu(ref.bn1(ref.conv1(imgd))))
            xs = [x0]
            for L in range(1, 5):
                x = xs[-1]
                for blk in getattr(ref, f"layer{L}"):
                    r = x if blk.downsample is None else blk.downsample(x)
                    x = F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x))))) + r)
                xs.append(x)

            def layer(L):
                def run():
                    x = xs[L - 1]
                    for blk in getattr(ref, f"layer{L}"):
                        r = x if blk.downsample is None else blk.downsample(x)
                        x = F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x))))) + r)
                    return x
                return run

            tp = list(ref(imgd))
            fpn = yr.feature_pyramid(hsd, tp)
            parts = {"stem + pool": lambda: ref.maxpool(F.relu(ref.bn1(ref.conv1(imgd)))),
                     **{f"layer{L}": layer(L) for L in range(1, 5)},
                     "fpn": lambda: yr.feature_pyramid(hsd, tp),
                     "protonet": lambda: yr.masknet(hsd, fpn[0]),
                     "heads": lambda: [yr.prediction_head(hsd, f, c["C"], c["k"]) for f in fpn]}
            breakdown = [{"part": n, "native_ms": round(native.get(n, 0.0), 4), "torch_ms": round(timed(fn, psteps, pwarm), 4)}
                         for n, fn in parts.items()]
        slower = [b["part"] for b in breakdown if b["native_ms"] > b["torch_ms"]]
        flops = geometry(eng.desc)["flops_per_frame"]
        ng = statistics.median(runs["fused_graph_ms"])
        res = {"metric": "ms per step, YOLACT from the image 550x550", "batch": B, "precision": a.precision,
               **{k: spread(v) for k, v in runs.items()},
               "torch_over_fused_graph": round(statistics.median(runs["torch_eager_ms"]) / ng, 3),
               "two_call_over_fused_graph": round(statistics.median(runs["two_call_eager_ms"]) / ng, 3),
               "gflop_per_frame": round(flops / 1e9, 3), "native_tflops": round(flops * B / ng / 1e9, 2),
               "slices": eng.slices(B), "knobs": knob_note, "rel_diff_native_vs_torch": err, "steps": a.steps,
               "warmup": a.warmup, "repeats": a.repeats, "slower_than_torch": slower,
               "frames_over_fused_graph": round(statistics.median(runs["frames_graph_ms"]) / ng, 4),
               "frames_graph_no_slower_than_fused_graph": statistics.median(runs["frames_graph_ms"]) <= ng,
               "frames_outputs_equal_torch_prep_outputs": frames_equal,
               "stem_pool_ms": {k: spread(v) for k, v in stem.items()}, "stem_pool_kernel": stem_kernel,
               "stem_u8_no_slower_than_fp32": statistics.median(stem["u8"]) <= statistics.median(stem["fp32"]),
               "library": a.lib or "default", "device": torch.cuda.get_device_name(0)}
        print(json.dumps(res), flush=True)
        res["parts"] = breakdown
        res["ops"] = [{"label": r[0], "ms": round(r[1], 4), "gflop": round(r[2] / 1e9, 4), "kernel": r[3]} for r in rows]
        results.append(res)
        del net, graph, head, fgraph, pgraph
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
