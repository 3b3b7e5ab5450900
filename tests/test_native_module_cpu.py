"""NativeModule (tauv_vision_amd/native.py) without a GPU, over every module that derives from it:
the state-dict metadata is torch's own, the parameter-version key moves with every way the
parameters can change, an invalid precision is refused, and the engine cache builds, keeps and
drops its one engine as documented (NativeEngine replaced by a counting stub)."""
import copy

import pytest
import torch
import torch.nn as nn

import tauv_vision_amd as tv
from recipe_yolact_head import head_case
from test_resnet18_cpu import small_config
from test_yolact_head_cpu import case_config
from tauv_vision_amd import _lib, native
from tauv_vision_amd.yolact import YolactConfig

HEAD = head_case("yolact_head_a")
DLA = ([2] * 5, [16] * 6, 2)  # the golden case r18_c16_b2_96x128


def _object_config():
    A = tv.AngleConfig
    return tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), False, False,
                                               None) for i in range(4)])


def _head_sizes(grow):
    return tuple((h + grow, w + grow) for h, w in HEAD["sizes"])


# name -> (constructor(precision), attribute names of its native children,
#          engine accessor(module, device, which of two sizes) or None for a module without a forward)
CLASSES = {
    "Masknet": (lambda p: tv.Masknet(YolactConfig(640, 360, (24, 48, 96, 192, 384), (1,), (0.1, 0.2), feature_depth=32,
                                                  n_prototype_masks=8), p), (),
                lambda m, d, i: m.engine(d, *((12, 20), (9, 17))[i])),
    "FeaturePyramid": (lambda p: tv.FeaturePyramid(HEAD["depths"], case_config(HEAD), p), (),
                       lambda m, d, i: m.engine(d, _head_sizes(i))),
    "PredictionHead": (lambda p: tv.PredictionHead(case_config(HEAD), p), (), None),
    "YolactHead": (lambda p: tv.YolactHead(HEAD["depths"], case_config(HEAD), p),
                   ("_feature_pyramid", "_masknet", "_prediction_head"),
                   lambda m, d, i: m.engine(d, _head_sizes(i))),
    "Resnet101Backbone": (lambda p: tv.Resnet101Backbone(None, p), (),
                          lambda m, d, i: m.engine(d, *((72, 88), (37, 51))[i])),
    "Yolact": (lambda p: tv.Yolact(small_config(72, 88), tv.Resnet101Backbone(None, p), p),
               ("_backbone", "_feature_pyramid", "_masknet", "_prediction_head"),
               lambda m, d, i: m._image_engine(d, *((72, 88), (37, 51))[i])[0]),
    "DLABackbone": (lambda p: tv.DLABackbone(*DLA, precision=p), (),
                    lambda m, d, i: m.engine(d, *((96, 128), (64, 96))[i])),
    "Centernet": (lambda p: tv.Centernet(tv.DLABackbone(*DLA), _object_config(), p), ("backbone",),
                  lambda m, d, i: m.engine(d, *((96, 128), (64, 96))[i])),
    "CenterpointDLA34": (lambda p: tv.CenterpointDLA34(_object_config(), p), (),
                         lambda m, d, i: m.engine(d, *((64, 96), (96, 128))[i])),
}
NAMES = list(CLASSES)


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_metadata_is_torchs_own(name):
    m = CLASSES[name][0]("fp32")
    before = m.state_dict()
    meta = copy.deepcopy(dict(before._metadata))
    assert meta and all(v == {"version": nn.Module._version} for v in meta.values())
    m.invalidate()
    m.float()
    m.load_state_dict(before)
    assert dict(before._metadata) == meta
    assert dict(m.state_dict()._metadata) == meta


@pytest.mark.parametrize("name", NAMES)
def test_version_key_changes_with_the_parameters(name):
    make, children, _ = CLASSES[name]
    m = make("fp32")
    assert isinstance(m, native.NativeModule)
    changes = [lambda: m.load_state_dict(m.state_dict()), m.float, lambda: m.set_precision("fp16")]
    for child in children:
        c = getattr(m, child)
        changes.append(lambda c=c: c.load_state_dict(c.state_dict()))
    for change in changes:
        key = m._version_key()
        assert m._version_key() == key
        change()
        assert m._version_key() != key
    below = [x for x in m.modules() if isinstance(x, native.NativeModule)]
    assert len(below) == 1 + len(children)
    assert m._version_key() == tuple(x._params_version for x in below)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_precision_is_refused(name):
    make = CLASSES[name][0]
    with pytest.raises(ValueError, match="precision"):
        make("nonsense")
    m = make("fp32")
    with pytest.raises(ValueError, match="precision"):
        m.set_precision("nonsense")
    assert m.precision == "fp32"
    assert m.set_precision("bf16") is m and m.precision == "bf16"


@pytest.mark.parametrize("name", [n for n in NAMES if CLASSES[n][2] is not None])
def test_engine_cache(name, monkeypatch):
    built = []

    class Engine:
        def __init__(self, desc, state_dict, device_index):
            built.append((desc, list(state_dict), device_index))

    monkeypatch.setattr(native, "NativeEngine", Engine)
    make, children, engine = CLASSES[name]
    m = make("fp32")
    dev = torch.device("cuda", 0)
    first = engine(m, dev, 0)
    assert engine(m, dev, 0) is first and len(built) == 1
    assert next(iter(m._engines.values())) is first
    seen = [first]

    def rebuilt():
        """The accessor builds a new engine, and that one is then the only one kept."""
        eng = engine(m, dev, 1)
        assert all(eng is not e for e in seen) and len(built) == len(seen) + 1
        assert engine(m, dev, 1) is eng and len(built) == len(seen) + 1
        assert list(m._engines.values()) == [eng]
        seen.append(eng)

    rebuilt()  # another size
    m.invalidate()
    rebuilt()
    m.set_precision("fp16")
    rebuilt()
    for child in children:
        c = getattr(m, child)
        c.load_state_dict(c.state_dict())
        rebuilt()
    assert all(index == 0 for _, _, index in built)
    own = list(m.state_dict())
    keys = built[-1][1]
    if name == "DLABackbone":
        assert keys == ["backbone." + k for k in own]
    elif name == "Resnet101Backbone":
        assert ["_feature_extractor." + k for k in keys] == own
    else:
        assert keys == own  # (Yolact: the whole state dict, the backbone's entries included)
    if name == "Yolact":
        assert any(k.startswith("_backbone.") for k in keys)
    if name in ("YolactHead", "Yolact"):  # YolactHead's own engine: everything but the backbone
        m.engine(dev, _head_sizes(0))
        keys = built[-1][1]
        assert keys == [k for k in own if not k.startswith("_backbone.")]
        assert len(keys) and len(m._engines) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is visible")
def test_require_gpu_refuses_without_a_device():
    with pytest.raises(RuntimeError, match="needs a gfx950 .MI355X. GPU; no HIP device is visible"):
        _lib.require_gpu()
