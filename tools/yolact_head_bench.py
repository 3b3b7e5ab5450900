"""Time the YOLACT neck + head at the benchmark geometry (550 x 550: backbone maps 128 x 69 x 69,
256 x 35 x 35, 512 x 18 x 18; F = 256, 7 classes, 8 prototypes, one aspect ratio, one trunk block,
two extra levels), batch 32:

  native   YolactHead (fp16 by default) with caller-owned outputs, as a replayed graph and as eager
           launches;
  torch    the same step in eager PyTorch-ROCm (tests/yolact_head_ref.py with the weights and maps
           cast to the same dtype) — what a user of the library had to run before.

Each is timed with device events around `--steps` iterations after `--warmup` (a synchronise ends
each window; at the defaults a window lasts 1.7 s or more), `--repeats` times, the three alternating,
on seeded inputs resident on the device: every number is reported as min / median / max over the
repeats. In separate passes: the per-op profile of the native step (one op per launch, HIP events),
and the same parts of the step in PyTorch (FPN, protonet, per level the head's blocks and its three
final convs with the permute / reshape / tanh), so that a native part slower than its PyTorch
counterpart is named (`slower_than_torch`). Prints one JSON line and writes it, with both
breakdowns, to --out.

Usage: python tools/yolact_head_bench.py [--batch 32] [--precision fp16] [--steps 300] [--warmup 20]
                                         [--repeats 3] [--out profiles/yolact_head/head_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolact_head", "head_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yolact_head_bench needs the MI355X: no HIP device is visible")

    import yolact_head_ref as yr
    from recipe_yolact_head import SCALES, VAR, head_case, head_inputs
    from tauv_vision_amd.weights import geometry
    from tauv_vision_amd.yolact import YolactConfig, YolactHead

    c = head_case("yolact_head_d")
    sd, _ = head_inputs(c)
    dev = torch.device("cuda", 0)
    B = a.batch
    g = torch.Generator(device=dev).manual_seed(2100)
    maps = [torch.randn((B, d, h, w), generator=g, device=dev) for d, (h, w) in zip(c["depths"], c["sizes"])]
    cfg = YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])
    head = YolactHead(c["depths"], cfg, precision=a.precision)
    head.load_state_dict(sd)

    # native: one eager step on the capture stream (workspaces, anchors), then capture and replay
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        first = head(maps)
        out = [torch.empty_like(first[0]), torch.empty_like(first[1]), torch.empty_like(first[2]),
               torch.empty((B, 4 * c["sizes"][0][0], 4 * c["sizes"][0][1], (c["k"] + 3) // 4 * 4), device=dev)]
        head(maps, out=out)
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        head(maps, out=out)

    # eager PyTorch-ROCm: the restatement in the same dtype (fp32 for the fp32 precisions)
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(a.precision, torch.float32)
    sdd = {k: v.to(dev, dt) if v.dtype.is_floating_point else v.to(dev) for k, v in sd.items()}
    mapsd = [m.to(dt) for m in maps]

    def torch_step():
        with torch.no_grad():
            return yr.yolact_head(sdd, mapsd, c["C"], c["k"])

    def native_eager():
        head(maps, out=out)

    runs = {"native_graph_ms": [], "native_eager_ms": [], "torch_eager_ms": []}
    for _ in range(a.repeats):  # alternating: a drift of the box hits all three alike
        runs["native_graph_ms"].append(timed(graph.replay, a.steps, a.warmup))
        runs["native_eager_ms"].append(timed(native_eager, a.steps, a.warmup))
        runs["torch_eager_ms"].append(timed(torch_step, a.steps, a.warmup))
    ref = torch_step()

    # the two steps compute the same thing (a loose sanity figure: both are low precision)
    err = {n: float((x.float() - y.float()).abs().max()) for n, x, y in
           (("cls", out[0], ref[0]), ("enc", out[1], ref[1]), ("coef", out[2], ref[2]),
            ("proto", out[3][..., :c["k"]].permute(0, 3, 1, 2), ref[3]))}

    # per part: the native profile's rows (one op per launch, one 32-frame workspace) against the same
    # part in PyTorch, each on its own (inputs resident, a synchronise around the window)
    eng = head.engine(dev, c["sizes"])
    eng.profile_multi(maps, out)  # (its workspace and first launches)
    rows = min((eng.profile_multi(maps, out) for _ in range(3)), key=lambda r: sum(x[1] for x in r))
    psteps, pwarm = max(20, a.steps // 3), 5
    with torch.no_grad():
        fpn = yr.feature_pyramid(sdd, mapsd)
        parts = {"fpn": (lambda: yr.feature_pyramid(sdd, mapsd),
                         lambda l: l.startswith("_feature_pyramid.") or l.startswith("pyramid ") or l.startswith("backbone map")),
                 "protonet": (lambda: yr.masknet(sdd, fpn[0]), lambda l: l.startswith("_masknet."))}
        hp = "_prediction_head."
        for i, f in enumerate(fpn):
            x = yr._blocks(sdd, hp, "_extra", f)
            lv = f"level {i} "
            parts[f"level {i} head blocks"] = (lambda f=f: yr._blocks(sdd, hp, "_extra", f),
                                               lambda l, lv=lv: l.startswith(lv) and "final" not in l and "raw heads" not in l)
            parts[f"level {i} final convs + reshape + tanh"] = (
                lambda x=x: (yr._conv(sdd, hp + "_classification_layer", x, padding=1).permute(0, 2, 3, 1).reshape(B, -1, c["C"] + 1),
                             yr._conv(sdd, hp + "_box_encoding_layer", x, padding=1).permute(0, 2, 3, 1).reshape(B, -1, 4),
                             torch.tanh(yr._conv(sdd, hp + "_mask_coeff_layer", x, padding=1).permute(0, 2, 3, 1).reshape(B, -1, c["k"]))),
                lambda l, lv=lv: l.startswith(lv) and ("final" in l or "raw heads" in l))
        breakdown = []
        for name, (fn, match) in parts.items():
            nat = sum(r[1] for r in rows if match(r[0]))
            breakdown.append({"part": name, "native_ms": round(nat, 4), "torch_ms": round(timed(fn, psteps, pwarm), 4)})
    slower = [b["part"] for b in breakdown if b["native_ms"] > b["torch_ms"]]

    flops = geometry(eng.desc)["flops_per_frame"]
    ng = statistics.median(runs["native_graph_ms"])
    res = {"metric": "ms per step, YOLACT neck + head + protonet 550x550", "batch": B, "precision": a.precision,
           **{k: spread(v) for k, v in runs.items()},
           "torch_over_native_graph": round(statistics.median(runs["torch_eager_ms"]) / ng, 3),
           "gflop_per_frame": round(flops / 1e9, 3), "native_tflops": round(flops * B / ng / 1e9, 2),
           "slices": eng.slices(B), "max_abs_diff_native_vs_torch": err, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "slower_than_torch": slower, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    res["parts"] = breakdown
    res["ops"] = [{"label": r[0], "ms": round(r[1], 4), "gflop": round(r[2] / 1e9, 4), "kernel": r[3]} for r in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
