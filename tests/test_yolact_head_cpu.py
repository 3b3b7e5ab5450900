"""YOLACT neck + head without a GPU: the planner's parameter layout against the reference modules'
own key lists, the torch restatement (tests/yolact_head_ref.py) pinned to the reference's goldens
(tests/golden/gen_golden_yolact_head.py), the desc validation, and the Python modules' state_dict
layout and refusals that need no device."""
import numpy as np
import pytest
import torch

import yolact_head_ref as yr
from helpers import golden
from recipe_yolact_head import HEAD_CASES, SCALES, VAR, head_case, head_inputs, head_layout, head_level_sizes, \
    head_sample_index
from tauv_vision_amd.weights import model_io, param_layout, yolact_head_desc

NAMES = [c["name"] for c in HEAD_CASES]


def case_desc(c, precision="fp32", fpn_only=False, **over):
    kw = dict(in_depths=c["depths"], map_sizes=c["sizes"], feature_depth=c["F"], n_fpn_downsample_layers=c["down"],
              n_classes=c["C"], n_prototype_masks=c["k"], n_aspect_ratios=len(c["ars"]), layers=c["layers"],
              precision=precision, fpn_only=fpn_only)
    kw.update(over)
    return yolact_head_desc(**kw)


def case_config(c):
    from tauv_vision_amd.yolact import YolactConfig
    return YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])


def case_inputs(c):
    """Seeded weights and maps, checked against the checksums the reference run stored."""
    sd, maps = head_inputs(c)
    g = golden(c["name"])
    got = np.array([[float(v.double().sum()), float(v.double().abs().sum())] if v.dtype.is_floating_point
                    else [float(v), 0.0] for v in sd.values()])
    assert np.allclose(got, g["weight_checksums"], rtol=1e-10, atol=1e-12), "seeded weight recipe drifted"
    got = np.array([[float(m.double().sum()), float(m.double().abs().sum())] for m in maps])
    assert np.allclose(got, g["input_checksum"], rtol=1e-10, atol=1e-9), "seeded inputs drifted"
    return sd, maps


@pytest.mark.parametrize("name", NAMES)
def test_param_layout_matches_reference(name):
    c = head_case(name)
    assert param_layout(case_desc(c)) == head_layout(c)
    fpn = [(k[len("_feature_pyramid."):], s) for k, s in head_layout(c) if k.startswith("_feature_pyramid.")]
    assert param_layout(case_desc(c, fpn_only=True)) == fpn


@pytest.mark.parametrize("name", NAMES)
def test_model_io_matches_reference_shapes(name):
    c, g = head_case(name), golden(name)
    A = g["cls"].shape[1]
    ins, outs = model_io(case_desc(c))
    assert ins == [(d, h, w) for d, (h, w) in zip(c["depths"], c["sizes"])]
    h, w = c["sizes"][0]
    kp = (c["k"] + 3) // 4 * 4
    assert outs == [(A, 1, c["C"] + 1, c["C"] + 1), (A, 1, 4, 4), (A, 1, c["k"], c["k"]), (4 * h, 4 * w, c["k"], kp)]
    assert tuple(g["proto_shape"]) == (c["batch"], c["k"], 4 * h, 4 * w)
    ins, outs = model_io(case_desc(c, fpn_only=True))
    assert outs == [(lh, lw, c["F"], c["F"]) for lh, lw in head_level_sizes(c)]
    assert A == sum(lh * lw for lh, lw in head_level_sizes(c)) * len(c["ars"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    c, g = head_case(name), golden(name)
    sd, maps = case_inputs(c)
    if c["full"]:
        for i, m in enumerate(maps):
            np.testing.assert_array_equal(m.numpy(), g[f"map{i}"])
    with torch.no_grad():
        cls, enc, coef, proto, fpn = yr.yolact_head(sd, maps, c["C"], c["k"])
    for got, key in ((cls, "cls"), (enc, "enc"), (coef, "coef")):
        np.testing.assert_allclose(got.numpy(), g[key], rtol=0, atol=1e-6)
    for i, f in enumerate(fpn):
        if f"fpn{i}" in g:
            np.testing.assert_allclose(f.numpy(), g[f"fpn{i}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(f.double().sum(dim=(0, 2, 3)).numpy(), g[f"fpn_chan_sum{i}"], rtol=1e-9, atol=1e-6)
    if c["full"]:
        np.testing.assert_allclose(proto.numpy(), g["proto"], rtol=0, atol=1e-6)
    else:
        np.testing.assert_array_equal(head_sample_index(c).numpy(), g["proto_sample_index"])
        np.testing.assert_allclose(proto.reshape(-1)[head_sample_index(c)].numpy(), g["proto_sample"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(proto.double().sum(dim=(0, 2, 3)).numpy(), g["proto_chan_sum"], rtol=1e-9, atol=1e-6)


def test_anchor_cat_matches_reference():
    from tauv_vision_amd.yolact import YolactHead
    for c in HEAD_CASES[:3]:
        head = YolactHead(c["depths"], case_config(c))
        assert head.level_sizes(c["sizes"]) == head_level_sizes(c)
        np.testing.assert_array_equal(head.anchor(head_level_sizes(c), torch.device("cpu")).numpy(),
                                      golden(c["name"])["anchor"])


def test_desc_validation():
    c = head_case("yolact_head_a")
    param_layout(case_desc(c))
    with pytest.raises((ValueError, RuntimeError), match="multiples of 4"):
        param_layout(case_desc(c, feature_depth=30))          # not whole 16-byte vectors of fp32
    with pytest.raises((ValueError, RuntimeError), match="multiples of 8"):
        param_layout(case_desc(c, precision="fp16", feature_depth=36))
    with pytest.raises((ValueError, RuntimeError), match="Bottleneck width"):
        param_layout(case_desc(c, precision="fp16", feature_depth=16))   # F / 4 = 4 < 8
    with pytest.raises(ValueError, match="2 map sizes for 3"):
        param_layout(case_desc(c, map_sizes=c["sizes"][:2]))
    with pytest.raises(ValueError, match="aspect ratio"):
        param_layout(case_desc(c, n_aspect_ratios=0))
    with pytest.raises(ValueError):
        param_layout(case_desc(c, map_sizes=((9, 11), (0, 6), (3, 3))))
    with pytest.raises(ValueError):
        param_layout(case_desc(c, n_fpn_downsample_layers=6))  # 9 levels > 8 outputs
    param_layout(case_desc(c, fpn_only=True, n_aspect_ratios=0))  # the FPN alone reads no head field


@pytest.mark.parametrize("name", NAMES[:3])
def test_modules_keep_reference_layout(name):
    from tauv_vision_amd.yolact import FeaturePyramid, PredictionHead, Yolact, YolactHead, yolact_head_state_dict
    c = head_case(name)
    cfg = case_config(c)
    layout = head_layout(c)
    head = YolactHead(c["depths"], cfg)
    assert [(k, tuple(v.shape)) for k, v in head.state_dict().items()] == layout
    fpn = FeaturePyramid(c["depths"], cfg)
    assert [("_feature_pyramid." + k, tuple(v.shape)) for k, v in fpn.state_dict().items()] == \
        [e for e in layout if e[0].startswith("_feature_pyramid.")]
    ph = PredictionHead(cfg)
    assert [("_prediction_head." + k, tuple(v.shape)) for k, v in ph.state_dict().items()] == \
        [e for e in layout if e[0].startswith("_prediction_head.")]
    # a reference Yolact state_dict: the backbone's entries are dropped by the helper; a missing key is reported
    sd, _ = head_inputs(c)
    full = dict(sd)
    full["_backbone._feature_extractor.conv1.weight"] = torch.zeros(4, 3, 7, 7)
    v0 = head._version_key()
    head.load_state_dict(yolact_head_state_dict(full))
    assert head._version_key() != v0
    for k, v in sd.items():
        assert torch.equal(head.state_dict()[k], v)
    with pytest.raises(RuntimeError, match="_backbone"):
        head.load_state_dict(full)
    short = {k: v for k, v in sd.items() if k != "_prediction_head._box_encoding_layer.bias"}
    with pytest.raises(RuntimeError, match="_box_encoding_layer.bias"):
        head.load_state_dict(short)
    with pytest.raises(RuntimeError, match="without a backbone"):
        Yolact(cfg, in_depths=c["depths"])(torch.zeros(1, 3, c["in_h"], c["in_w"]))
    with pytest.raises(ValueError, match="expected 3 backbone maps"):
        head((torch.zeros(1, 16, 4, 4),))
    with pytest.raises(RuntimeError, match="YolactHead"):
        ph(torch.zeros(1, c["F"], 4, 4))


def e2e_case():
    """The end-to-end case with the seed its generator found."""
    from recipe_yolact_head import E2E_CASE
    return dict(E2E_CASE, seed=int(golden(E2E_CASE["name"])["seed"]))


def test_e2e_fixture_margins_and_restatement():
    """The stored NMS indices follow from the stored head tensors with both margins above 1e-3 (so an
    error of 1e-4 cannot change them), and the restatement + the oracle's post-processing reproduce
    the reference's boxes, indices and masks."""
    from oracle import ref_yolact as ry
    from recipe_yolact_head import E2E_MARGIN, E2E_NMS, nms_margins
    c = e2e_case()
    g = golden(c["name"])
    assert param_layout(case_desc(c)) == head_layout(c)
    conf_margin, iou_margin, n = nms_margins(torch.from_numpy(g["cls"]), torch.from_numpy(g["box"]), *E2E_NMS, ry.iou_matrix)
    assert conf_margin > E2E_MARGIN and iou_margin > E2E_MARGIN
    assert n == int(g["n_candidates"]) and 2 <= len(g["det"]) < n  # something kept, something suppressed
    sd, maps = case_inputs(c)
    with torch.no_grad():
        cls, enc, coef, proto, _ = yr.yolact_head(sd, maps, c["C"], c["k"])
    for got, key in ((cls, "cls"), (enc, "enc"), (coef, "coef"), (proto, "proto")):
        np.testing.assert_allclose(got.numpy(), g[key], rtol=0, atol=1e-6)
    box = ry.box_decode(enc, torch.from_numpy(g["anchor"]), VAR)
    np.testing.assert_allclose(box.numpy(), g["box"], rtol=4e-7, atol=1e-6)
    det = ry.nms(cls, box, *E2E_NMS)
    np.testing.assert_array_equal(det.numpy(), g["det"])
    np.testing.assert_allclose(ry.assemble_mask(proto[0], coef[0, det], box[0, det]).numpy(), g["mask"], rtol=0, atol=1e-6)
