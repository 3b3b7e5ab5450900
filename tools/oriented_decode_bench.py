"""Oriented decode: what tv_decode_angles adds to tv_decode, against eager PyTorch doing the same work.

Workload: a 120 x 160 output grid, 4 labels of periods 2 pi, pi, pi / 2 and pi / 3 on all three axes, K = 100,
score threshold 0 (every record is live), at B = 1 and B = 64. The prediction is what the native models
return: channel slices of one fp32 NHWC head tensor (heatmap, size, offset, roll / pitch / yaw bin and
offset: 32 channels), seeded normal values; the bin logits are drawn under the condition of
tests/angle_decode_ref.py, so that no cell's bin choice hangs on the last bit of an fp32 exp.

  decode         tv_decode alone (DeviceDecoder);
  decode_angles  tv_decode, then tv_decode_angles into the same packed buffer (DeviceAngleDecoder);
  torch          on the records tv_decode left on the device: label / y / x from the flat index, the gather
                 of the 3 x 2 heads at the K peaks, the package's torch angle_decode per axis, the period
                 table and the NaN mask past the counts — about 60 torch kernels.
Each is the HIP-event time of a replayed graph of `--inner` calls, median over `--repeats` replays
(tools/localize_bench.py's scheme); `torch_eager_us` is the same torch code launched op by op, HIP events
around `--inner` calls. `max_diff` is the largest circular distance between the torch and the device angles.
Prints one line per case and a final JSON line, also written to --out."""
import argparse
import json
import os
import sys
from math import pi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tauv-vision_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import angle_decode_ref as ref  # noqa: E402
import tauv_vision_amd as tv  # noqa: E402
from localize_bench import graph_us  # noqa: E402
from tauv_vision_amd.centernet import prediction_from_nhwc  # noqa: E402

H, W, K = 120, 160, 100
PERIODS = (2 * pi, pi, pi / 2, pi / 3)
AXES = ("roll", "pitch", "yaw")


def object_config():
    A = tv.AngleConfig
    return tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(True, p), A(True, p), A(True, p), False, False, None)
                               for i, p in enumerate(PERIODS)])


def torch_angles(records, counts, pred, table):
    """The same [B, K, 3] as tv_decode_angles, in eager torch on the device."""
    B = records.shape[0]
    flat = records[..., 7].long()
    label = flat // (H * W)
    y, x = flat // W % H, flat % W
    b = torch.arange(B, device=records.device)[:, None].expand(B, K)
    live = torch.arange(K, device=records.device)[None, :] < counts[:, None]
    out = []
    for a, axis in enumerate(AXES):
        bins, off = getattr(pred, axis + "_bin")[b, y, x], getattr(pred, axis + "_offset")[b, y, x]
        ang = tv.angle_decode(bins, off, 2 * pi, 0.0) * (table[a][label] / (2 * pi))
        out.append(torch.where(live, ang, torch.full_like(ang, float("nan"))))
    return torch.stack(out, dim=-1)


def eager_us(fn, inner, repeats):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(repeats + 2):
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3 / inner)
    return float(np.median(times[2:]))


def case(B, dev, inner, repeats):
    oc = object_config()
    mc = tv.ModelConfig([], [], 4 * H, 4 * W, 2, pi / 3)
    g = torch.Generator().manual_seed(17 + B)
    head = torch.randn((B, H, W, sum(tv.get_head_channels(oc))), generator=g).to(dev)
    pred = prediction_from_nhwc(head, oc)
    rng = np.random.default_rng(B)
    for axis in AXES:
        getattr(pred, axis + "_bin").copy_(torch.from_numpy(ref.conditioned_bins(rng, (B, H, W))))
    C = oc.n_labels
    dec = tv.DeviceDecoder(B, C, H, W, K, dev, angles=True)
    ang = tv.DeviceAngleDecoder(B, K, oc, dev, out=dec.angles)
    table = ang.theta_range

    def decode():
        dec(pred.heatmap, pred.size, pred.offset, None, 0, mc.downsample_ratio, mc.in_h, mc.in_w, 0.0)

    def decode_angles():
        decode()
        ang(dec.records, dec.counts, pred)

    decode_angles()
    torch.cuda.synchronize()
    want = torch_angles(dec.records, dec.counts, pred, table)
    assert int(dec.counts.min()) == K and not torch.isnan(dec.angles).any()
    period = table.t()[(dec.records[..., 7].long() // (H * W))]  # [B, K, 3]
    d = (dec.angles - want).abs() % period
    max_diff = float(torch.minimum(d, period - d).max())
    r = dict(B=B, decode_us=graph_us(decode, dev, inner, repeats),
             decode_angles_us=graph_us(decode_angles, dev, inner, repeats),
             torch_graph_us=graph_us(lambda: torch_angles(dec.records, dec.counts, pred, table), dev, inner, repeats),
             torch_eager_us=eager_us(lambda: torch_angles(dec.records, dec.counts, pred, table), inner, repeats),
             max_diff=max_diff)
    r["angles_us"] = r["decode_angles_us"] - r["decode_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="calls per replayed graph")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode", "oriented_decode_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = []
    for B in (1, 64):
        r = case(B, dev, args.inner, args.repeats)
        cases.append(r)
        print(f"B={B:2d}: tv_decode {r['decode_us']:8.1f} us, + tv_decode_angles {r['decode_angles_us']:8.1f} us "
              f"(+{r['angles_us']:.1f}); torch on the same records {r['torch_graph_us']:8.1f} us in a graph, "
              f"{r['torch_eager_us']:8.1f} us eager; max difference {r['max_diff']:.2e}", flush=True)
    line = json.dumps(dict(tool="oriented_decode_bench", grid=[H, W], labels=len(PERIODS), K=K, inner=args.inner,
                           repeats=args.repeats, cases=cases))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
