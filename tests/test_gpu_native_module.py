"""The engine cache of NativeModule (tauv_vision_amd/native.py) on the GPU, for the two classes
without a reload test of their own: Masknet at the geometry of the golden protonet_f32_k8_b2_12x20
and the stand-alone DLABackbone at the golden case r18_c16_b2_96x128, both fp32. A repeated forward
reuses the engine and gives the same bits; new parameters and a new precision each build a new one."""
import pytest
import torch

from helpers import case_by_name, case_input, case_state_dict
from recipe import protonet_case, protonet_inputs
from tauv_vision_amd.weights import seeded_state_dict

pytestmark = pytest.mark.gpu


def _masknet():
    from tauv_vision_amd.yolact import Masknet, YolactConfig
    c = protonet_case("protonet_f32_k8_b2_12x20")
    sd, x = protonet_inputs(c)
    m = Masknet(YolactConfig(640, 360, (24, 48, 96, 192, 384), (1,), (0.1, 0.2), feature_depth=c["F"],
                             n_prototype_masks=c["k"]))
    m.load_state_dict(sd)
    return m.cuda().eval(), x.cuda()


def _backbone():
    import tauv_vision_amd as tv
    name = "r18_c16_b2_96x128"
    case = case_by_name(name)
    bb = tv.DLABackbone(case["heights"], case["channels"], case["downsamples"])
    bb.load_state_dict({k[len("backbone."):]: v for k, v in case_state_dict(name).items() if k.startswith("backbone.")})
    return bb.cuda().eval(), case_input(name).cuda()


def _engine(m):
    assert len(m._engines) == 1
    return next(iter(m._engines.values()))


@pytest.mark.parametrize("make", [_masknet, _backbone], ids=["Masknet", "DLABackbone"])
def test_reload_and_precision_build_a_new_engine(make):
    m, x = make()
    first = m(x).clone()
    eng = _engine(m)
    assert torch.equal(m(x), first) and _engine(m) is eng
    m.load_state_dict(seeded_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], conv_seed=7,
                                        aux_seed=8))
    second = m(x).clone()
    eng2 = _engine(m)
    assert eng2 is not eng
    assert second.shape == first.shape and not torch.equal(second, first)
    assert m.set_precision("fp16") is m
    m(x)
    assert _engine(m) is not eng2 and _engine(m) is not eng
    assert _engine(m).desc.compute_dtype == 1  # fp16
