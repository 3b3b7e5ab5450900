"""CenterNet training loss: tauv_vision_amd.loss.loss against the reference's algorithm on the same GPU,
the dense kernel's bandwidth, and the parity figures behind tests/test_gpu_centernet_loss.py.

Workload: the 90 x 160 map (360 x 640 input, two downsamples), 8 objects and 12 keypoint instances per
sample, B = 32, a synthetic prediction in the reference model's layout (NCHW heatmaps, NHWC views of
NCHW heads):
  torpedo    4 labels, 4 keypoints, no angle or depth heads (the torpedo config's heads);
  allheads   the same plus roll / pitch / yaw and depth.
One step is loss(...) and total.backward(), wall time between two device synchronisations.
  baseline   tests/centernet_loss_ref.py's loss_ref on fp32 CUDA tensors: the reference's own sequence of
             torch ops and Python loops, one indexing op per object and head (the targets are built by
             the oracle on the host and uploaded, which is cheaper than the reference's own per-object
             launches: the baseline is not handicapped);
  new        tauv_vision_amd.loss.loss on the same fp32 tensors, and on fp16 copies.
Three alternating rounds of `--steps` steps after `--warmup`; a round's figure is its median, a side's the
median of its three rounds, `*_spread_ms` is max - min of a side's three. `ok` says whether the new fp32
step is not above the baseline by more than the baseline's own spread.

  dense      tv_centernet_loss_dense alone on those inputs (fp32 and fp16): HIP-event time of a replayed
             graph of `--inner` launches, median over `--repeats` replays (tools/localize_bench.py's
             scheme), against the bytes it moves: every heatmap / affinity logit read once, every
             gradient element written once (the object heads' zero fill included).
  parity     per fixture and term e_ref = |T_ref - T64| / S and e_dev = |T_dev - T64| / S, per tensor
             max |g_ref - g64|, max |g_dev - g64| and max |g64| (tests/test_gpu_centernet_loss.py's
             quantities), written to profiles/loss/parity.json.
Prints one line per figure and a final JSON line, also written to --out."""
import argparse
import ctypes
import json
import os
import sys
import time
from math import pi
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import centernet_loss_ref as R  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402
from localize_bench import graph_us  # noqa: E402
from tauv_vision_amd import _lib, loss as L  # noqa: E402

IN_H, IN_W, DS, N_OBJ, N_INST, LABELS = 360, 640, 2, 8, 12, 4
DENSE = ("heatmap", "keypoint_heatmap", "keypoint_affinity")


def make_case(all_heads, B, dev, seed=31):
    g = torch.Generator().manual_seed(seed)
    mc = tv.ModelConfig([2] * 5, [16] * 6, IN_H, IN_W, DS, pi / 3)
    H, W = mc.out_h, mc.out_w
    tc = SimpleNamespace(heatmap_focal_loss_a=2.0, heatmap_focal_loss_b=4.0, keypoint_heatmap_sigma=2.0,
                         keypoint_affinity_sigma=3.0, loss_lambda_keypoint_heatmap=1.0,
                         loss_lambda_keypoint_affinity=0.1, loss_lambda_size=1.0, loss_lambda_offset=1.0,
                         loss_lambda_angle=0.5, loss_lambda_depth=0.2)
    angle = lambda m: SimpleNamespace(modulo=m if all_heads else None)  # noqa: E731
    oc = SimpleNamespace(n_labels=LABELS, n_keypoints=LABELS,
                         configs=[SimpleNamespace(roll=angle(pi / 2), pitch=angle(pi), yaw=angle(2 * pi))] * LABELS)
    r = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    truth = L.PoseSample(valid=r(B, N_OBJ) < 0.8, label=torch.randint(0, LABELS, (B, N_OBJ), generator=g),
                         center=r(B, N_OBJ, 2), size=r(B, N_OBJ, 2) * 0.3, roll=r(B, N_OBJ) * 6, pitch=r(B, N_OBJ) * 6,
                         yaw=r(B, N_OBJ) * 6, depth=r(B, N_OBJ) * 4 + 0.3, keypoint_valid=r(B, N_INST) < 0.85,
                         keypoint_label=torch.randint(0, LABELS, (B, N_INST), generator=g),
                         keypoint_center=r(B, N_INST, 2),
                         keypoint_object_index=torch.randint(0, N_OBJ, (B, N_INST), generator=g))
    truth = L.PoseSample(**{k: None if v is None else v.to(dev) for k, v in vars(truth).items()})
    widths = {"heatmap": LABELS, "keypoint_heatmap": LABELS, "keypoint_affinity": 2 * LABELS, "size": 2, "offset": 2}
    if all_heads:
        widths.update({f"{a}_{k}": 4 for a in ("roll", "pitch", "yaw") for k in ("bin", "offset")}, depth=1)
    nchw = {h: (3.0 if h in DENSE[:2] else 1.0) * torch.randn((B, w, H, W), generator=g) for h, w in widths.items()}
    return mc, tc, oc, truth, nchw


def views(nchw, dtype, dev):
    leaf = {h: t.to(dev, dtype).requires_grad_(True) for h, t in nchw.items()}
    view = {h: None for h in R.HEADS}
    for h, t in leaf.items():
        view[h] = t if h in DENSE[:2] else t.unflatten(1, (LABELS, 2)) if h == "keypoint_affinity" \
            else t.permute(0, 2, 3, 1)
    return leaf, SimpleNamespace(**view)


def wall_ms(step, steps, warmup):
    for _ in range(warmup):
        step()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def step_case(name, all_heads, B, dev, steps, warmup):
    mc, tc, oc, truth, nchw = make_case(all_heads, B, dev)
    sides = {}
    for side, dtype in (("baseline", torch.float32), ("new", torch.float32), ("new_fp16", torch.float16)):
        leaf, view = views(nchw, dtype, dev)

        def step(side=side, leaf=leaf, view=view):
            for t in leaf.values():
                t.grad = None
            total = R.loss_ref(view, truth, mc, tc, oc)[0]["total"] if side == "baseline" else \
                L.loss(view, truth, mc, tc, oc, None).total
            total.backward()
            return total
        sides[side] = step
    base, new = float(sides["baseline"]()), float(sides["new"]())
    assert abs(base - new) <= 1e-4 * abs(base), (base, new)  # the two sides compute the same loss
    rounds = {s: [] for s in sides}
    for _ in range(3):
        for s, step in sides.items():
            rounds[s].append(wall_ms(step, steps, warmup))
    med = {s: float(np.median(v)) for s, v in rounds.items()}
    spread = {s: max(v) - min(v) for s, v in rounds.items()}
    return dict(shape=name, B=B, map=[mc.out_h, mc.out_w], steps=steps, warmup=warmup, total=base,
                baseline_ms=med["baseline"], new_ms=med["new"], new_fp16_ms=med["new_fp16"],
                baseline_rounds_ms=rounds["baseline"], new_rounds_ms=rounds["new"],
                new_fp16_rounds_ms=rounds["new_fp16"], baseline_spread_ms=spread["baseline"],
                new_spread_ms=spread["new"], new_fp16_spread_ms=spread["new_fp16"],
                ratio=med["baseline"] / med["new"], ratio_fp16=med["baseline"] / med["new_fp16"],
                ok=med["new"] <= med["baseline"] + spread["baseline"])


def dense_case(name, all_heads, B, dtype, dev, inner, repeats):
    """The dense launch alone, on the description and buffers of a real loss() call."""
    mc, tc, oc, truth, nchw = make_case(all_heads, B, dev)
    leaf, view = views(nchw, dtype, dev)
    calls, run = [], L._Call.run

    def keep(self, tensors, want):
        calls.append((self, tensors))
        return run(self, tensors, want)
    L._Call.run = keep
    try:
        L.loss(view, truth, mc, tc, oc, None)
    finally:
        L._Call.run = run
    call, tensors = calls[0]
    lib, ref, n = _lib.lib(), ctypes.byref(call.desc), ctypes.c_int64()
    _lib.check(lib.tv_centernet_loss_workspace_size(ref, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)

    def launch():
        _lib.check(lib.tv_centernet_loss_dense(ref, ctypes.c_void_p(ws.data_ptr()), n.value, _lib.stream_of(dev)))
    us = graph_us(launch, dev, inner, repeats)
    esize = leaf["heatmap"].element_size()
    read = sum(t.numel() for h, t in leaf.items() if h in DENSE) * esize
    written = sum(t.numel() for t in leaf.values()) * esize
    return dict(shape=name, B=B, dtype=str(dtype).split(".")[-1], us=us, bytes_read=read, bytes_written=written,
                gb_per_s=(read + written) / us / 1e3)


def parity():
    import test_gpu_centernet_loss as T
    out = {}
    for name, dtype in [(n, torch.float32) for n in R.CASES] + [(T.A, torch.float16), (T.A, torch.bfloat16)]:
        v64, S, g64, v32, g32 = T.restated(name, dtype)
        vals, grads = T.device(name, dtype)
        terms = {}
        for t, want in v64.items():
            if t == "heatmap_alone" or np.isnan(want):
                continue
            s = S[t] if S[t] else 1.0
            terms[t] = dict(f64=float(want), S=float(S[t]), e_ref=abs(float(v32[t]) - want) / s,
                            e_dev=abs(float(vals[t]) - want) / s)
        tensors = {}
        for h, want in g64.items():
            ok = ~np.isnan(want)
            tensors[h] = dict(max_g64=float(np.abs(want[ok]).max()), err_ref=float(np.abs(g32[h][ok] - want[ok]).max()),
                              err_dev=float(np.abs(grads[h][ok] - want[ok]).max()), nan=int((~ok).sum()))
        out[f"{name}/{str(dtype).split('.')[-1]}"] = dict(terms=terms, gradients=tensors)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "loss_bench.json"))
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "loss", "parity.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    par = parity()
    with open(args.parity_out, "w") as f:
        json.dump(par, f, indent=1, sort_keys=True)
        f.write("\n")
    for case, v in par.items():
        worst = max(v["terms"].items(), key=lambda kv: kv[1]["e_dev"])
        print(f"parity {case}: worst term {worst[0]} e_dev {worst[1]['e_dev']:.3g} (e_ref {worst[1]['e_ref']:.3g})",
              flush=True)
    dense, steps = [], []
    for name, all_heads in (("torpedo", False), ("allheads", True)):
        for dtype in (torch.float32, torch.float16):
            r = dense_case(name, all_heads, args.batch, dtype, dev, args.inner, args.repeats)
            dense.append(r)
            print(f"dense {name} B={r['B']} {r['dtype']}: {r['us']:.1f} us, {(r['bytes_read'] + r['bytes_written']) / 1e6:.1f} MB, "
                  f"{r['gb_per_s']:.0f} GB/s", flush=True)
    for name, all_heads in (("torpedo", False), ("allheads", True)):
        r = step_case(name, all_heads, args.batch, dev, args.steps, args.warmup)
        steps.append(r)
        print(f"step {name} B={r['B']}: baseline {r['baseline_ms']:.2f} ms (spread {r['baseline_spread_ms']:.2f}), new "
              f"{r['new_ms']:.3f} ms (spread {r['new_spread_ms']:.3f}), fp16 {r['new_fp16_ms']:.3f} ms, ratio "
              f"{r['ratio']:.0f}x / {r['ratio_fp16']:.0f}x, ok {r['ok']}", flush=True)
    line = json.dumps(dict(tool="centernet_loss_bench", input=[IN_H, IN_W], objects=N_OBJ, keypoint_instances=N_INST,
                           labels=LABELS, steps=steps, dense=dense, ok=all(r["ok"] for r in steps)))
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
