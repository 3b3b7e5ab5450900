"""Training augmentation timing probe: DeviceAugmenter (csrc/augment.hip, two launches) at the reference's
training shapes — YOLACT: B = 24 frames of 360 x 640 to 360 x 640 with the seg map, records drawn from the
TrainConfig of yolact/scripts/train.py:51-81; CenterNet: B = 32 (configs/samples_torpedo.py:19) frames of
360 x 640, no seg map, records from sample_centernet_params. HIP-event time of a replayed graph of `--inner`
calls, median over `--repeats` replays. Bytes are computed from the shapes: the source frames (and seg map)
read once, the fp32 planes (and seg map) written; the achieved rate is given as a share of the 6.29 TB/s a
float4 copy reaches on this part and of the 8.0 TB/s specification.

Baselines, in this tool's own words:
  * the same definition composed from eager PyTorch-ROCm ops on the same device (F.grid_sample for the
    warp and the seg map, elementwise colour ops, torch.randn for the noise, F.avg_pool2d over reflect
    padding per kernel size), timed the same way (graph replay of the same number of calls). It runs the
    HSV round trip and the noise for EVERY frame, where the kernel skips either for a frame whose record
    does not ask for it (the JSON counts those frames): the ratio includes that saving;
  * the numpy restatement (tests/augment_ref.py, fp32) on the host, ONE image, host clock, scaled to B.
Neither is the reference's albumentations pipeline, which is not installed here: not measured.
Prints one line per case and a final JSON line (also written to --out)."""
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
import torch.nn.functional as F  # noqa: E402

from tauv_vision_amd import augment as A  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_COPY, HBM_SPEC = 6.29e12, 8.0e12  # bytes / s: measured float4 copy, specification
YOLACT_TRAIN = SimpleNamespace(  # yolact/scripts/train.py:51-81
    channel_shuffle_p=0, color_jitter_p=1, color_jitter_brightness=0.2, color_jitter_contrast=0.2,
    color_jitter_saturation=0.2, color_jitter_hue=0.2, gaussian_noise_p=1.0, gaussian_noise_var_limit=(10.0, 50.0),
    horizontal_flip_p=0.5, vertical_flip_p=0.5, blur_limit=(3, 7), blur_p=0.5, ssr_p=1, ssr_shift_limit=(-0.1, 0.1),
    ssr_scale_limit=(-0.1, 0.1), ssr_rotate_limit=(-30, 30), perspective_p=1, perspective_scale_limit=(0.0, 0.25),
    min_visibility=0.0)


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


def frames_of(B, hw, dev, seed):
    """Smooth frames (a bicubic enlargement of a random field plus a little pixel noise), as camera frames are."""
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.rand((B, 3, hw[0] // 16 + 3, hw[1] // 16 + 3), generator=g, device=dev)
    up = F.interpolate(low, hw, mode="bicubic", align_corners=False) + 0.02 * torch.randn((B, 3) + hw, generator=g,
                                                                                         device=dev)
    return (up.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class Eager:
    """The definition from eager torch ops (a timing baseline: grid_sample's own border handling and
    torch.randn's own generator, so its pixels are not the kernel's)."""

    def __init__(self, params, dev):
        rec = params.records.to(dev)
        B = rec.shape[0]
        self.B, (self.Hs, self.Ws), (self.Hd, self.Wd) = B, params.src_hw, params.dst_hw
        self.minv = rec[:, :9].view(B, 3, 3)
        self.perm = rec[:, 9:12].long()
        col = lambda i: rec[:, i].view(B, 1, 1, 1)  # noqa: E731
        self.br, self.ct, self.sat, self.hue, self.ss, self.vs, self.sigma = (col(i) for i in range(12, 19))
        ks = [int(v) for v in params.records[:, 19]]
        self.groups = {k: torch.tensor([i for i, v in enumerate(ks) if v == k], device=dev) for k in sorted(set(ks) - {1})}
        self.n531 = torch.tensor([5.0, 3.0, 1.0], device=dev).view(1, 3, 1, 1)
        ys, xs = torch.meshgrid(torch.arange(self.Hd, device=dev) + 0.5, torch.arange(self.Wd, device=dev) + 0.5,
                                indexing="ij")
        self.xy1 = torch.stack([xs, ys, torch.ones_like(xs)], -1).view(1, -1, 3)
        self.mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
        self.std = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
        self.gray_w = torch.tensor([0.299, 0.587, 0.114], device=dev).view(1, 3, 1, 1)

    def inside_share(self):
        """The share of destination pixels whose source position lies in the frame."""
        q = self.xy1 @ self.minv.transpose(1, 2)
        w = q[..., 2]
        u, v = q[..., 0] / w, q[..., 1] / w
        return float(((w > 0) & (u >= 0) & (u < self.Ws) & (v >= 0) & (v < self.Hs)).float().mean())

    def __call__(self, frames, seg):
        B, Hd, Wd = self.B, self.Hd, self.Wd
        src = frames.permute(0, 3, 1, 2).float()
        src = torch.gather(src, 1, self.perm.view(B, 3, 1, 1).expand(-1, -1, self.Hs, self.Ws))
        q = self.xy1 @ self.minv.transpose(1, 2)
        w = q[..., 2]
        u, v = q[..., 0] / w, q[..., 1] / w
        inside = ((w > 0) & (u >= 0) & (u < self.Ws) & (v >= 0) & (v < self.Hs)).view(B, 1, Hd, Wd)
        grid = torch.stack([u / self.Ws * 2 - 1, v / self.Hs * 2 - 1], -1).view(B, Hd, Wd, 2)
        c = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=False)
        mu = ((src * self.br).clamp(0, 255) * self.gray_w).sum(1, keepdim=True).mean((2, 3), keepdim=True)
        c = (c * self.br).clamp(0, 255)
        c = (self.ct * c + (1 - self.ct) * mu).clamp(0, 255)
        c = (self.sat * c + (1 - self.sat) * (c * self.gray_w).sum(1, keepdim=True)).clamp(0, 255)
        n = c / 255
        mx, mn = n.amax(1, keepdim=True), n.amin(1, keepdim=True)
        d = mx - mn
        ds = torch.where(d > 0, d, torch.ones_like(d))
        r, g, b = n[:, 0:1], n[:, 1:2], n[:, 2:3]
        h = torch.where(mx == r, (g - b) / ds, torch.where(mx == g, (b - r) / ds + 2, (r - g) / ds + 4))
        h = torch.where(d > 0, h / 6, torch.zeros_like(h)) + self.hue
        h = h - torch.floor(h)
        s = (torch.where(mx > 0, d / torch.where(mx > 0, mx, torch.ones_like(mx)), torch.zeros_like(mx)) + self.ss) \
            .clamp(0, 1)
        val = (mx + self.vs).clamp(0, 1)
        kk = torch.remainder(self.n531 + 6 * h, 6)
        c = (val - val * s * torch.minimum(torch.minimum(kk, 4 - kk), torch.ones_like(kk)).clamp_min(0)) * 255
        c = (c + self.sigma * torch.randn_like(c)).clamp(0, 255)
        c = torch.where(inside, c, torch.zeros_like(c))
        out = c.clone()
        for k, idx in self.groups.items():
            out.index_copy_(0, idx, F.avg_pool2d(F.pad(c.index_select(0, idx), (k // 2,) * 4, mode="reflect"), k, 1))
        out = torch.where(inside, out, torch.zeros_like(out))
        img = (out / 255 - self.mean) / self.std
        if seg is None:
            return img, None
        sg = F.grid_sample(seg.unsqueeze(1).float(), grid, mode="nearest", padding_mode="border", align_corners=False)
        return img, torch.where(inside, sg, torch.full_like(sg, 254.0)).to(torch.uint8)[:, 0]


def case(name, B, hw, with_seg, params, dev, args):
    frames = frames_of(B, hw, dev, seed=B)
    seg = None
    if with_seg:
        seg = torch.randint(0, 6, (B, 1, hw[0] // 40, hw[1] // 40), device=dev,
                            generator=torch.Generator(device=dev).manual_seed(B + 1)).float()
        seg = F.interpolate(seg, hw, mode="nearest").to(torch.uint8)[:, 0].contiguous()
    aug = A.DeviceAugmenter(B, hw, hw, MEAN, STD, dev)
    aug.load(params)
    us = graph_us(lambda: aug(frames, seg, None, 1234), dev, args.inner, args.repeats)
    px = B * hw[0] * hw[1]
    nbytes = px * 3 + px * 12 + (2 * px if with_seg else 0)
    eager = Eager(params, dev)
    eager_us = graph_us(lambda: eager(frames, seg), dev, args.inner, args.repeats)
    import augment_ref as R
    fr, sg = frames[:1].cpu().numpy(), None if seg is None else seg[:1].cpu().numpy()
    t0 = time.perf_counter()
    R.augment(fr, sg, params.records[:1].numpy(), 1234, MEAN, STD, hw, np.float32)
    host_s = time.perf_counter() - t0
    rec = params.records
    return dict(case=name, B=B, src=list(hw), dst=list(hw), seg=with_seg, us=us, bytes=nbytes,
                tbps=nbytes / us * 1e-6, share_of_copy_rate=nbytes / (us * 1e-6) / HBM_COPY,
                share_of_spec=nbytes / (us * 1e-6) / HBM_SPEC, eager_us=eager_us, speedup_over_eager=eager_us / us,
                numpy_one_image_ms=host_s * 1e3, numpy_batch_ms_scaled=host_s * 1e3 * B,
                frames_with_blur=int((rec[:, A.BLUR_K] > 1).sum()), frames_with_noise=int((rec[:, A.NOISE_SIGMA] > 0).sum()),
                frames_with_contrast=int((rec[:, A.CONTRAST] != 1).sum()),
                frames_with_hsv=int(((rec[:, A.HUE] != 0) | (rec[:, A.SAT_SHIFT] != 0) | (rec[:, A.VAL_SHIFT] != 0)).sum()),
                inside_share=eager.inside_share())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20, help="calls per replayed graph")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the MI355X: no HIP device is visible")
    dev = torch.device("cuda", 0)
    hw = (360, 640)
    model = SimpleNamespace(in_h=hw[0], in_w=hw[1])
    g = torch.Generator().manual_seed(0)
    results = [case("yolact B=24 360x640 seg", 24, hw, True, A.sample_yolact_params(YOLACT_TRAIN, model, hw, 24, g), dev,
                    args),
               case("centernet B=32 360x640", 32, hw, False, A.sample_centernet_params(hw, hw, 32, g), dev, args)]
    for r in results:
        print(f"{r['case']:28s}: {r['us']:9.1f} us {r['bytes'] / 1e6:8.2f} MB {r['tbps']:6.3f} TB/s "
              f"({r['share_of_copy_rate']:.1%} of the copy rate) | eager torch {r['eager_us']:10.1f} us "
              f"({r['speedup_over_eager']:.1f}x) | numpy on the host {r['numpy_one_image_ms']:.0f} ms per image", flush=True)
    line = json.dumps(dict(tool="augment_bench", inner=args.inner, repeats=args.repeats, results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
