"""Generate the YOLACT neck + head goldens (tests/golden/recipe_yolact_head.py HEAD_CASES).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference modules
src/tauv_vision/yolact/model/{config,feature_pyramid,prediction_head,masknet,anchors}.py read-only.
The .npz / .json files hold seeded inputs, key lists and the reference's outputs; no reference source.

prediction_head.py imports torchvision.models.resnet.Bottleneck and torchvision is not installed
here, so a stand-in module with torchvision's parameter layout and forward is registered first
(conv1, bn1, conv2, bn2, conv3, bn3; bias-free 1x1 / 3x3 / 1x1 convs of width `planes`, expansion
4, stride 1, no downsample: out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + x)) — the
same terms as the DeformConv2d stand-in of gen_golden_dla34.py. BatchNorm runs in eval().

Per case: the reference FeaturePyramid, Masknet and PredictionHead are built, loaded with
seeded_state_dict over their own key order (Yolact's registration order: `_feature_pyramid.`,
`_masknet.`, `_prediction_head.`), and run as Yolact.forward runs them (model.py:34-60). Stored:
the key list (yolact_head_layouts.json), weight checksums, every FPN level, the three head tensors,
the anchors and the prototypes (case D: inputs regenerated from the seed, the prototypes as a seeded
sample + per-channel sums, the FPN levels as per-channel sums + the two smallest in full, so that the
file stays under 1 MiB).

The end-to-end case (yolact_head_e2e) also stores box_decode, nms(100, 0.5, 0.05) and assemble_mask of
the reference outputs, from the reference's own functions; its classification layer's background bias
is raised by the recipe's `bg_bias` and its seed is searched so that both margins of the NMS decision
exceed 1e-3 (gen_e2e asserts them; the seed found is stored).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_yolact_head.py [case ...]
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
sys.path.insert(0, HERE)
from recipe_yolact_head import (E2E_CASE, E2E_MARGIN, E2E_NMS, HEAD_CASES, SCALES, VAR, head_inputs,  # noqa: E402
                                head_sample_index, nms_margins)


class Bottleneck(nn.Module):
    """torchvision.models.resnet.Bottleneck(inplanes, planes) with its defaults."""
    expansion = 4

    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + x)


def install_stand_in():
    if "torchvision" in sys.modules:
        return
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    resnet = types.ModuleType("torchvision.models.resnet")
    resnet.Bottleneck = Bottleneck
    tv.models, models.resnet = models, resnet
    sys.modules.update({"torchvision": tv, "torchvision.models": models, "torchvision.models.resnet": resnet})


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def ref_config(ModelConfig, c):
    fields = {f: None for f in ModelConfig.__dataclass_fields__}
    fields.update(in_w=c["in_w"], in_h=c["in_h"], feature_depth=c["F"], n_classes=c["C"], n_prototype_masks=c["k"],
                  n_prediction_head_layers=c["layers"][0], n_classification_layers=c["layers"][1],
                  n_box_layers=c["layers"][2], n_mask_layers=c["layers"][3], n_fpn_downsample_layers=c["down"],
                  anchor_scales=SCALES, anchor_aspect_ratios=c["ars"], box_variances=VAR)
    return ModelConfig(**fields)


def run_reference(c, mods):
    """The reference modules on the case's seeded weights and maps, as Yolact.forward runs them after
    the backbone (model.py:34-60) -> (config, layout, state_dict, maps, fpn, proto, cls, enc, coef, anchor)."""
    ModelConfig, FeaturePyramid, PredictionHead, Masknet, get_anchor = mods[:5]
    cfg = ref_config(ModelConfig, c)
    net = nn.Module()
    net._feature_pyramid = FeaturePyramid(c["depths"], cfg)
    net._masknet = Masknet(cfg)
    net._prediction_head = PredictionHead(cfg)
    net.eval()
    layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd, maps = head_inputs(c, layout)
    net.load_state_dict(sd)
    with torch.no_grad():
        fpn = net._feature_pyramid(tuple(maps))
        proto = net._masknet(fpn[0])
        parts = [net._prediction_head(f) for f in fpn]
        anchor = torch.cat([get_anchor(i, tuple(f.size()[2:4]), cfg) for i, f in enumerate(fpn)], dim=1)
    cls, enc, coef = (torch.cat([p[j] for p in parts], dim=1) for j in range(3))
    return cfg, layout, sd, maps, fpn, proto, cls, enc, coef, anchor


def gen_e2e(mods, layouts):
    """The end-to-end case (recipe_yolact_head.E2E_CASE): the reference outputs through the reference
    box_decode -> nms -> assemble_mask. Seeds are tried from the case's on until both margins of the
    NMS decision exceed E2E_MARGIN (asserted before the file is written), some candidate is suppressed
    and some kept; the seed found is stored."""
    box_decode, nms, assemble_mask, iou_matrix = mods[5:]
    top_k, iou_thr, conf_thr = E2E_NMS
    for seed in range(E2E_CASE["seed"], E2E_CASE["seed"] + 200):
        c = dict(E2E_CASE, seed=seed)
        cfg, layout, sd, maps, fpn, proto, cls, enc, coef, anchor = run_reference(c, mods)
        box = box_decode(enc, anchor, cfg)
        n_all = int((torch.softmax(cls[0], -1)[:, 1:].max(-1).values >= conf_thr).sum())
        if not 4 <= n_all < top_k:
            continue
        conf_margin, iou_margin, n = nms_margins(cls, box, top_k, iou_thr, conf_thr, iou_matrix)
        det = nms(cls, box, top_k, iou_thr, conf_thr)
        if conf_margin > E2E_MARGIN and iou_margin > E2E_MARGIN and 2 <= len(det) < n:
            break
    else:
        raise SystemExit("no seed with the NMS margins found")
    assert conf_margin > E2E_MARGIN, conf_margin   # consecutive sorted confidences, distance to the threshold
    assert iou_margin > E2E_MARGIN, iou_margin     # every pairwise IoU the decision reads vs the IoU threshold
    layouts[c["name"]] = [[k, list(s)] for k, s in layout]
    mask = assemble_mask(proto[0], coef[0, det], box[0, det])
    chk = np.array([[float(v.double().sum()), float(v.double().abs().sum())] if v.dtype.is_floating_point
                    else [float(v), 0.0] for v in sd.values()])
    out = dict(seed=np.array(seed), bg_bias=np.array(c["bg_bias"]), weight_checksums=chk, cls=cls.numpy(), enc=enc.numpy(),
               coef=coef.numpy(), anchor=anchor.numpy(), proto=proto.numpy(), box=box.numpy(), det=det.numpy(),
               mask=mask.numpy(), n_candidates=np.array(n), margins=np.array([conf_margin, iou_margin]),
               input_checksum=np.array([[float(m.double().sum()), float(m.double().abs().sum())] for m in maps]))
    save_npz(os.path.join(HERE, c["name"] + ".npz"), out)
    print(c["name"], "seed", seed, "candidates", n, "kept", det.tolist(), "margins", conf_margin, iou_margin)


def gen_case(c, mods, layouts):
    cfg, layout, sd, maps, fpn, proto, cls, enc, coef, anchor = run_reference(c, mods)
    layouts[c["name"]] = [[k, list(s)] for k, s in layout]
    chk = np.array([[float(v.double().sum()), float(v.double().abs().sum())] if v.dtype.is_floating_point
                    else [float(v), 0.0] for v in sd.values()])
    out = dict(weight_checksums=chk, cls=cls.numpy(), enc=enc.numpy(), coef=coef.numpy(), anchor=anchor.numpy(),
               proto_shape=np.array(proto.shape), proto_chan_sum=proto.double().sum(dim=(0, 2, 3)).numpy(),
               input_checksum=np.array([[float(m.double().sum()), float(m.double().abs().sum())] for m in maps]))
    for i, f in enumerate(fpn):
        out[f"fpn_chan_sum{i}"] = f.double().sum(dim=(0, 2, 3)).numpy()
    if c["full"]:
        out["proto"] = proto.numpy()
        for i, m in enumerate(maps):
            out[f"map{i}"] = m.numpy()
        for i, f in enumerate(fpn):
            out[f"fpn{i}"] = f.numpy()
    else:
        idx = head_sample_index(c)
        out.update(proto_sample_index=idx.numpy(), proto_sample=proto.reshape(-1)[idx].numpy())
        for i, f in enumerate(fpn):  # the small levels in full, per-channel sums (above) of every level
            if f.numel() <= 32768:
                out[f"fpn{i}"] = f.numpy()
    save_npz(os.path.join(HERE, c["name"] + ".npz"), out)
    print(c["name"], "anchors", anchor.shape[1], "cls range", float(cls.min()), float(cls.max()), "proto",
          tuple(proto.shape), float(proto.min()), float(proto.max()))


def main():
    sys.dont_write_bytecode = True
    install_stand_in()
    sys.path.insert(0, REF_SRC)
    from tauv_vision.yolact.model.config import ModelConfig
    from tauv_vision.yolact.model.feature_pyramid import FeaturePyramid
    from tauv_vision.yolact.model.prediction_head import PredictionHead
    from tauv_vision.yolact.model.masknet import Masknet
    from tauv_vision.yolact.model.anchors import get_anchor
    from tauv_vision.yolact.model.boxes import box_decode, iou_matrix
    from tauv_vision.yolact.model.nms import nms
    from tauv_vision.yolact.model.masks import assemble_mask
    mods = (ModelConfig, FeaturePyramid, PredictionHead, Masknet, get_anchor, box_decode, nms, assemble_mask, iou_matrix)
    want = set(sys.argv[1:])
    path = os.path.join(HERE, "yolact_head_layouts.json")
    layouts = {}
    if want and os.path.exists(path):
        with open(path) as f:
            layouts = json.load(f)
    for c in HEAD_CASES:
        if not want or c["name"] in want:
            gen_case(c, mods, layouts)
    if not want or E2E_CASE["name"] in want:
        gen_e2e(mods, layouts)
    with open(path, "w") as f:
        json.dump({k: layouts[k] for k in sorted(layouts)}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
