"""The ResNet-18 backbone and the whole-model arch without a GPU: the planner's parameter layout
against the restated torchvision module tree (tests/resnet18_ref.py; parity with torchvision itself is
not pinned, see its docstring), model_io shapes, desc validation, and the Python modules' state_dict
layout, strict loading and the refusals that need no device."""
import pytest
import torch

import resnet18_ref as rr
from recipe_yolact_head import head_case, head_inputs, head_layout
from test_yolact_head_cpu import case_config
from tauv_vision_amd.weights import model_io, param_layout, resnet18_desc, yolact_desc, yolact_head_desc

BB = "_backbone._feature_extractor."
# a small whole model on the native backbone: F = 32, k = 8, one aspect ratio, two extra levels (head
# case A's head fields; its 16 / 32 / 64-channel maps are not a ResNet-18's, so its weights do not apply)
SMALL = dict(F=32, C=7, k=8, ars=(1,), layers=(1, 0, 0, 0), down=2)


def small_desc(in_h, in_w, precision="fp32", **over):
    kw = dict(in_h=in_h, in_w=in_w, feature_depth=SMALL["F"], n_fpn_downsample_layers=SMALL["down"],
              n_classes=SMALL["C"], n_prototype_masks=SMALL["k"], n_aspect_ratios=len(SMALL["ars"]),
              layers=SMALL["layers"], precision=precision)
    kw.update(over)
    return yolact_desc(**kw)


def small_config(in_h, in_w):
    from recipe_yolact_head import SCALES, VAR
    from tauv_vision_amd.yolact import YolactConfig
    return YolactConfig(in_w, in_h, SCALES, SMALL["ars"], VAR, SMALL["F"], SMALL["k"], SMALL["C"], *SMALL["layers"],
                        SMALL["down"])


def ref_layout():
    return [(k, tuple(v.shape)) for k, v in rr.ResNet18Ref().state_dict().items()]


def test_param_layout_matches_restated_module():
    want = ref_layout()
    assert len(want) == 120 and not any(k.startswith("fc.") for k, _ in want)
    assert param_layout(resnet18_desc()) == want
    full = param_layout(small_desc(72, 88))
    assert [(k[len(BB):], s) for k, s in full if k.startswith(BB)] == want
    assert [k for k, _ in full[:len(want)]] == [BB + k for k, _ in want]  # the backbone first (model.py:25-29)
    head = yolact_head_desc((128, 256, 512), [(9, 11), (5, 6), (3, 3)], SMALL["F"], SMALL["down"], SMALL["C"],
                            SMALL["k"], 1, SMALL["layers"])
    assert full[len(want):] == param_layout(head)


def test_strict_loading_both_ways():
    from tauv_vision_amd.yolact import Resnet101Backbone
    bb = Resnet101Backbone(None)
    assert bb.depths == (128, 256, 512)
    assert [(k, tuple(v.shape)) for k, v in bb.state_dict().items()] == \
        [("_feature_extractor." + k, s) for k, s in ref_layout()]
    sd = rr.seeded_resnet18_state_dict(3)
    v0 = bb._params_version
    bb.load_state_dict({"_feature_extractor." + k: v for k, v in sd.items()}, strict=True)
    assert bb._params_version != v0
    for k, v in sd.items():
        assert torch.equal(bb.state_dict()["_feature_extractor." + k], v)
    ref = rr.ResNet18Ref()
    ref.load_state_dict(bb.backbone_state_dict(), strict=True)
    for k, v in sd.items():
        assert torch.equal(ref.state_dict()[k], v)
    with pytest.raises(RuntimeError, match="layer3.0.downsample.1.running_var"):
        bb.load_state_dict({"_feature_extractor." + k: v for k, v in sd.items()
                            if k != "layer3.0.downsample.1.running_var"})


@pytest.mark.parametrize("hw,sizes", [((550, 550), [(69, 69), (35, 35), (18, 18)]),
                                      ((360, 640), [(45, 80), (23, 40), (12, 20)]),
                                      ((37, 51), [(5, 7), (3, 4), (2, 2)])])
def test_model_io_shapes(hw, sizes):
    from tauv_vision_amd.yolact import Resnet101Backbone
    assert Resnet101Backbone.map_sizes(*hw) == sizes
    ins, outs = model_io(resnet18_desc(*hw))
    assert ins == [(3, *hw)]
    assert outs == [(h, w, c, c) for (h, w), c in zip(sizes, (128, 256, 512))]
    ins, outs = model_io(small_desc(*hw))
    assert ins == [(3, *hw)]
    head = yolact_head_desc((128, 256, 512), sizes, SMALL["F"], SMALL["down"], SMALL["C"], SMALL["k"], 1,
                            SMALL["layers"])
    assert outs == model_io(head)[1]


def test_the_restatement_follows_the_conv_arithmetic():
    """The restated module's own tap shapes are the planner's (floor-mode pooling, padding 1 / 3)."""
    m = rr.ResNet18Ref()
    with torch.no_grad():
        taps = m(torch.zeros(1, 3, 37, 51))
    assert [tuple(t.shape) for t in taps] == [(1, 128, 5, 7), (1, 256, 3, 4), (1, 512, 2, 2)]


def test_desc_validation():
    # a non-empty image always reaches layer4 ((x - 1) // 2 + 1 >= 1): the sizes too small for it are the empty ones
    for hw in ((0, 64), (64, 0), (-3, 5)):
        with pytest.raises(ValueError, match="in_h, in_w"):
            param_layout(resnet18_desc(*hw))
        with pytest.raises(ValueError, match="in_h, in_w"):
            model_io(small_desc(*hw))
    param_layout(resnet18_desc(1, 1))
    with pytest.raises((ValueError, RuntimeError), match="multiples of 4"):
        param_layout(small_desc(72, 88, feature_depth=30))
    with pytest.raises((ValueError, RuntimeError), match="Bottleneck width"):
        param_layout(small_desc(72, 88, precision="fp16", feature_depth=16))
    with pytest.raises(ValueError, match="aspect ratio"):
        param_layout(small_desc(72, 88, n_aspect_ratios=0))
    with pytest.raises(ValueError):
        param_layout(small_desc(72, 88, n_fpn_downsample_layers=6))


def test_whole_state_dict_loads_strictly_and_round_trips():
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact
    cfg = small_config(72, 88)
    c = dict(head_case("yolact_head_a"), depths=(128, 256, 512))
    head_keys = [(k, s) for k, s in param_layout(small_desc(72, 88)) if not k.startswith(BB)]
    # (case A's own head keys, but for the lateral convs' input depths)
    assert [k for k, _ in head_keys] == [k for k, _ in head_layout(head_case("yolact_head_a"))]
    sd, _ = head_inputs(c, layout=head_keys)
    full = {BB + k: v for k, v in rr.seeded_resnet18_state_dict(5).items()}
    full.update(sd)
    net = Yolact(cfg, backbone=Resnet101Backbone(cfg))
    assert net.in_depths == (128, 256, 512)
    v0 = net._version_key()
    net.load_state_dict(full, strict=True)
    assert net._version_key() != v0
    back = net.state_dict()
    assert set(back) == set(full)
    for k, v in full.items():
        assert torch.equal(back[k], v), k
    other = Yolact(cfg, backbone=Resnet101Backbone(cfg))
    other.load_state_dict(back, strict=True)
    with pytest.raises(RuntimeError, match="layer1.0.conv1.weight"):
        net.load_state_dict({k: v for k, v in full.items() if k != BB + "layer1.0.conv1.weight"})
    # set_precision covers the backbone, and the backbone's version is part of the engine key
    net.set_precision("fp16")
    assert net._backbone.precision == net._masknet.precision == "fp16"
    v1 = net._version_key()
    net._backbone.load_state_dict(net._backbone.state_dict())
    assert net._version_key() != v1
    with pytest.raises(ValueError):
        net.set_precision("fp8")


def test_refusals_that_need_no_device():
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact
    cfg = case_config(head_case("yolact_head_a"))
    with pytest.raises(RuntimeError, match="without a backbone"):
        Yolact(cfg, in_depths=(16, 32, 64))(torch.zeros(1, 3, 72, 88))
    bb = Resnet101Backbone(cfg)
    for bad in (torch.zeros(3, 72, 88), torch.zeros(1, 4, 72, 88)):
        with pytest.raises(ValueError, match="expected img"):
            bb(bad)
        with pytest.raises(ValueError, match="expected img"):
            Yolact(small_config(72, 88), backbone=bb)(bad)
    with pytest.raises(ValueError, match="in_depths"):
        Yolact(cfg, backbone=bb, in_depths=(16, 32, 64))
