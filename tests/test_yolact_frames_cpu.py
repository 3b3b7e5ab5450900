"""The YOLACT frame entry points without a GPU: every argument error of forward_frames, detect,
detection_records and YolactDetector is a ValueError raised before the "needs a GPU" error, and
YolactConfig's new fields come last with the ImageNet defaults, so positional construction is unchanged."""
import dataclasses

import pytest
import torch

from test_resnet18_cpu import SMALL, small_config


def _net(cfg=None):
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact
    cfg = cfg or small_config(72, 88)
    return Yolact(cfg, backbone=Resnet101Backbone(cfg))


def _frames(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype)


BAD_FRAMES = [_frames(2, 72, 88, 3, dtype=torch.float32), _frames(2, 72, 88, 3, dtype=torch.int8),
              _frames(2, 72, 88, 4), _frames(2, 3, 72, 88), _frames(72, 88), _frames(1, 2, 72, 88, 3), _frames(2, 0, 88, 3)]


@pytest.mark.parametrize("i", range(len(BAD_FRAMES)))
def test_bad_frames_are_value_errors(i):
    net = _net()
    bad = BAD_FRAMES[i]
    for call in (lambda: net.forward_frames(bad), lambda: net._backbone.forward_frames(bad),
                 lambda: net.detect(bad, 20, 0.5, 0.3)):
        with pytest.raises(ValueError, match="uint8"):
            call()
    with pytest.raises(ValueError, match="torch tensor"):
        net.forward_frames(bad.numpy())


def test_bad_size_top_k_and_camera_are_value_errors():
    net = _net()
    ok = _frames(2, 72, 88, 3)
    for size in ((72,), (72, 88, 3), (0, 88)):
        with pytest.raises(ValueError, match="size"):
            net.forward_frames(ok, size=size)
        with pytest.raises(ValueError, match="size"):
            net._backbone.forward_frames(ok, size=size)
    with pytest.raises(ValueError, match="top_k"):
        net.detect(ok, 0, 0.5, 0.3)
    with pytest.raises(ValueError, match="go together"):
        net.detect(ok, 20, 0.5, 0.3, depth=torch.zeros(90, 120, dtype=torch.uint16))
    with pytest.raises(ValueError, match="camera"):
        net.detect(ok, 20, 0.5, 0.3, depth=torch.zeros(90, 120, dtype=torch.uint16), camera=(1.0, 1.0, 0.0))
    with pytest.raises(ValueError, match="uint16"):
        net.detect(ok, 20, 0.5, 0.3, depth=torch.zeros(90, 120), camera=(1.0, 1.0, 0.0, 0.0))


def test_other_normalisation_constants_are_refused():
    from tauv_vision_amd.yolact import YolactDetector
    ok = _frames(2, 72, 88, 3)
    for change in (dict(img_mean=(0.5, 0.456, 0.406)), dict(img_stddev=(0.229, 0.224, 0.25))):
        net = _net(dataclasses.replace(small_config(72, 88), **change))
        for call in (lambda: net.forward_frames(ok), lambda: net._backbone.forward_frames(ok),
                     lambda: net.detect(ok, 20, 0.5, 0.3),
                     lambda: YolactDetector(net, 2, (72, 88), 20, "cuda")):
            with pytest.raises(ValueError, match="ImageNet"):
                call()
    # the ImageNet values in any sequence type are the defaults
    net = _net(dataclasses.replace(small_config(72, 88), img_mean=[0.485, 0.456, 0.406]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a gfx950"):
            net.forward_frames(ok)


def test_good_arguments_reach_the_gpu_error():
    if torch.cuda.is_available():  # (with a GPU these calls run: tests/test_gpu_yolact_frames.py)
        return
    from tauv_vision_amd.yolact import YolactDetector
    net = _net()
    ok = _frames(2, 72, 88, 3)
    for call in (lambda: net.forward_frames(ok), lambda: net.forward_frames(ok[0], size=(36, 44)),
                 lambda: net._backbone.forward_frames(ok), lambda: net.detect(ok, 20, 0.5, 0.3),
                 lambda: YolactDetector(net, 2, (72, 88), 20, "cuda")):
        with pytest.raises(RuntimeError, match="needs a gfx950"):
            call()


def test_detector_argument_errors():
    from tauv_vision_amd.yolact import Yolact, YolactDetector, YolactHead
    net = _net()
    with pytest.raises(ValueError, match="native backbone"):
        YolactDetector(YolactHead((128, 256, 512), small_config(72, 88)), 2, (72, 88), 20, "cuda")
    with pytest.raises(ValueError, match="native backbone"):
        YolactDetector(Yolact(small_config(72, 88), backbone=torch.nn.Identity()), 2, (72, 88), 20, "cuda")
    for B, top_k, hw in ((0, 20, (72, 88)), (2, 0, (72, 88)), (2, 20, (72,)), (2, 20, (72, 0))):
        with pytest.raises(ValueError, match="B >= 1"):
            YolactDetector(net, B, hw, top_k, "cuda")
    with pytest.raises(ValueError, match="native backbone"):
        Yolact(small_config(72, 88), backbone=torch.nn.Identity()).detect(_frames(2, 72, 88, 3), 20, 0.5, 0.3)


def test_detection_records_argument_errors():
    from tauv_vision_amd.yolact import detection_records
    B, A, C1, n = 2, 9, 4, 5
    good = dict(classification=torch.zeros(B, A, C1), box=torch.zeros(B, A, 4),
                det=torch.zeros(B, n, dtype=torch.int64), counts=torch.zeros(B, dtype=torch.int32))
    bad = [("det", good["det"].int(), "int64"), ("counts", good["counts"].long(), "int32"),
           ("classification", good["classification"].half(), "float32"), ("box", good["box"].double(), "float32"),
           ("box", [0.0], "torch tensor"),
           ("classification", torch.zeros(A, C1), "need classification"), ("det", torch.zeros(n, dtype=torch.int64), "need classification"),
           ("box", torch.zeros(B, A, 5), "belong together"), ("box", torch.zeros(B, A + 1, 4), "belong together"),
           ("det", torch.zeros(B + 1, n, dtype=torch.int64), "belong together"),
           ("counts", torch.zeros(B + 1, dtype=torch.int32), "belong together"),
           ("classification", torch.zeros(B, A, 1), "2 classes")]
    for name, value, match in bad:
        with pytest.raises(ValueError, match=match):
            detection_records(**dict(good, **{name: value}))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a gfx950"):
            detection_records(**good)


def test_config_positional_construction_is_unchanged():
    from recipe_yolact_head import SCALES, VAR
    from tauv_vision_amd.yolact import IMAGENET_MEAN, IMAGENET_STDDEV, YolactConfig
    names = [f.name for f in dataclasses.fields(YolactConfig)]
    assert names[-2:] == ["img_mean", "img_stddev"]
    assert names[:13] == ["in_w", "in_h", "anchor_scales", "anchor_aspect_ratios", "box_variances", "feature_depth",
                          "n_prototype_masks", "n_classes", "n_prediction_head_layers", "n_classification_layers",
                          "n_box_layers", "n_mask_layers", "n_fpn_downsample_layers"]
    # as bench.py and the existing tests build it
    c = YolactConfig(88, 72, SCALES, SMALL["ars"], VAR, SMALL["F"], SMALL["k"], SMALL["C"], *SMALL["layers"], SMALL["down"])
    assert (c.in_w, c.in_h, c.n_fpn_downsample_layers) == (88, 72, SMALL["down"])
    assert c.img_mean == IMAGENET_MEAN == (0.485, 0.456, 0.406) and c.img_stddev == IMAGENET_STDDEV == (0.229, 0.224, 0.225)
    assert YolactConfig(88, 72, SCALES, (1.0,), VAR).img_mean == IMAGENET_MEAN
