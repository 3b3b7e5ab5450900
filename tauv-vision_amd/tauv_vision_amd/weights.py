"""Reference state_dict layout (from the native planner) and a seeded synthetic-weight
recipe (no checkpoints travel)."""
import ctypes
import math

import torch

from . import _lib


(ARCH_CENTERNET, ARCH_DLA34, ARCH_PROTONET, ARCH_CENTERNET_BACKBONE, ARCH_YOLACT_HEAD, ARCH_YOLACT_FPN, ARCH_RESNET18,
 ARCH_YOLACT) = range(8)
RESNET18_DEPTHS = (128, 256, 512)  # layer2.1.bn2, layer3.1.bn2, layer4.1.bn2 (yolact/model/backbone.py:21-32)


def model_desc(heights, channels, downsamples, head_channels, in_h=64, in_w=64, precision="fp32",
               arch=ARCH_CENTERNET):
    if len(channels) != len(heights) + 1:
        raise ValueError("backbone_channels must have len(backbone_heights) + 1 entries")
    if len(heights) > 8 or len(head_channels) > 16:
        raise ValueError("too many backbone levels or heads")
    d = _lib.ModelDesc()
    d.n_levels = len(heights)
    for i, h in enumerate(heights):
        d.heights[i] = int(h)
    for i, c in enumerate(channels):
        d.channels[i] = int(c)
    d.downsamples = int(downsamples)
    d.n_heads = len(head_channels)
    for i, c in enumerate(head_channels):
        d.head_channels[i] = int(c)
    d.in_h, d.in_w = int(in_h), int(in_w)
    if precision not in _lib.DTYPES:
        raise ValueError(f"precision must be one of {sorted(_lib.DTYPES)}")
    d.compute_dtype = _lib.DTYPES[precision]
    d.arch = int(arch)
    return d


def dla34_desc(head_channels, in_h=64, in_w=64, precision="fp32"):
    """CenterpointDLA34 (centerpoint_dla.py:544-578): the DLA-34 structure is fixed."""
    return model_desc([], [16], 2, head_channels, in_h, in_w, precision, arch=ARCH_DLA34)


def protonet_desc(feature_depth, n_prototype_masks, fpn_h=8, fpn_w=8, precision="fp32"):
    """YOLACT Masknet (masknet.py:8-55) over an fpn[0] map of fpn_h x fpn_w."""
    return model_desc([], [feature_depth], 0, [n_prototype_masks], fpn_h, fpn_w, precision, arch=ARCH_PROTONET)


def yolact_head_desc(in_depths, map_sizes, feature_depth, n_fpn_downsample_layers, n_classes=0, n_prototype_masks=0,
                     n_aspect_ratios=0, layers=(0, 0, 0, 0), precision="fp32", fpn_only=False):
    """Everything of Yolact.forward after the backbone (ARCH_YOLACT_HEAD) or its FeaturePyramid alone
    (fpn_only: ARCH_YOLACT_FPN) over backbone maps of `in_depths` channels and `map_sizes` [(h, w)].
    `layers` = (n_prediction_head_layers, n_classification_layers, n_box_layers, n_mask_layers).
    The field encoding is documented at tv_model_desc in include/tauv_vision_amd.h."""
    if len(in_depths) > 8 or len(map_sizes) > 8 or len(layers) != 4:
        raise ValueError("at most 8 backbone maps; four layer counts")
    heads = [] if fpn_only else [n_prototype_masks, n_classes]
    d = model_desc(list(layers), [feature_depth] * 5, n_fpn_downsample_layers, heads, 0, 0, precision,
                   arch=ARCH_YOLACT_FPN if fpn_only else ARCH_YOLACT_HEAD)
    d.n_levels = len(in_depths)
    for i in range(9):
        d.channels[i] = 0
    d.channels[0] = int(feature_depth)
    for i, c in enumerate(in_depths):
        d.channels[1 + i] = int(c)
    d.n_maps = len(map_sizes)
    for i, (h, w) in enumerate(map_sizes):
        d.map_h[i], d.map_w[i] = int(h), int(w)
    d.n_aspect_ratios = int(n_aspect_ratios)
    return d


def resnet18_desc(in_h=64, in_w=64, precision="fp32"):
    """The YOLACT backbone (ARCH_RESNET18: torchvision's resnet18 tapped at layer2.1.bn2, layer3.1.bn2,
    layer4.1.bn2) over an in_h x in_w image; the structure is fixed."""
    return model_desc([], [64], 0, [], in_h, in_w, precision, arch=ARCH_RESNET18)


def yolact_desc(in_h, in_w, feature_depth, n_fpn_downsample_layers, n_classes, n_prototype_masks, n_aspect_ratios,
                layers=(0, 0, 0, 0), precision="fp32"):
    """The whole Yolact.forward from an in_h x in_w image (ARCH_YOLACT): the ResNet-18 backbone, then the
    head fields of yolact_head_desc over its taps (depths fixed at RESNET18_DEPTHS, sizes by the conv
    arithmetic). Keys: the whole reference state_dict."""
    d = yolact_head_desc(RESNET18_DEPTHS, [], feature_depth, n_fpn_downsample_layers, n_classes, n_prototype_masks,
                         n_aspect_ratios, layers, precision)
    d.arch = ARCH_YOLACT
    d.in_h, d.in_w = int(in_h), int(in_w)
    return d


def model_io(desc):
    """The caller's buffers of a desc, per frame: ([(C, H, W)] of the fp32 NCHW inputs,
    [(H, W, C, cpad)] of the fp32 NHWC outputs)."""
    n_in, n_out = ctypes.c_int32(), ctypes.c_int32()
    ins, outs = ((ctypes.c_int32 * 3) * 8)(), ((ctypes.c_int32 * 4) * 8)()
    _lib.check(_lib.lib().tv_model_io(ctypes.byref(desc), ctypes.byref(n_in), ins, ctypes.byref(n_out), outs),
               "model io")
    return [tuple(ins[i]) for i in range(n_in.value)], [tuple(outs[i]) for i in range(n_out.value)]


def param_layout(desc):
    """[(key, shape)] in reference registration (state_dict) order."""
    L = _lib.lib()
    n = ctypes.c_int32()
    _lib.check(L.tv_model_param_count(ctypes.byref(desc), ctypes.byref(n)), "param layout")
    out = []
    name = ctypes.create_string_buffer(512)
    shape = (ctypes.c_int64 * 4)()
    nd = ctypes.c_int32()
    for i in range(n.value):
        _lib.check(L.tv_model_param_info(ctypes.byref(desc), i, name, 512, shape, ctypes.byref(nd)), "param info")
        out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
    return out


def geometry(desc):
    L = _lib.lib()
    fl = ctypes.c_double()
    oh, ow, oc, ocp = (ctypes.c_int32() for _ in range(4))
    _lib.check(L.tv_model_geometry(ctypes.byref(desc), ctypes.byref(fl), ctypes.byref(oh), ctypes.byref(ow),
                                   ctypes.byref(oc), ctypes.byref(ocp)), "geometry")
    return dict(flops_per_frame=fl.value, out_h=oh.value, out_w=ow.value, out_channels=oc.value,
                out_cpad=ocp.value)


def seeded_state_dict(layout, conv_seed=0, aux_seed=1):
    """Deterministic weights for a key layout: conv / conv-transpose weights xavier-uniform
    (generator conv_seed); from generator aux_seed in key order: BN gamma U(.75,1.25),
    beta N(0,.1^2), running_mean N(0,.1^2), running_var U(.75,1.25), conv bias U(-.1,.1)."""
    g_conv = torch.Generator().manual_seed(conv_seed)
    g_aux = torch.Generator().manual_seed(aux_seed)
    names = {k for k, _ in layout}
    sd = {}
    for key, shape in layout:
        prefix, leaf = key.rsplit(".", 1)
        bn = (prefix + ".running_mean") in names
        shape = tuple(shape)
        if leaf == "num_batches_tracked":
            sd[key] = torch.tensor(0, dtype=torch.long)
        elif leaf == "running_mean":
            sd[key] = torch.randn(shape, generator=g_aux) * 0.1
        elif leaf == "running_var":
            sd[key] = torch.rand(shape, generator=g_aux) * 0.5 + 0.75
        elif len(shape) == 4:
            bound = math.sqrt(6.0 / ((shape[0] + shape[1]) * shape[2] * shape[3]))
            sd[key] = (torch.rand(shape, generator=g_conv) * 2.0 - 1.0) * bound
        elif bn and leaf == "weight":
            sd[key] = torch.rand(shape, generator=g_aux) * 0.5 + 0.75
        elif bn and leaf == "bias":
            sd[key] = torch.randn(shape, generator=g_aux) * 0.1
        elif leaf == "bias":
            sd[key] = (torch.rand(shape, generator=g_aux) * 2.0 - 1.0) * 0.1
        else:
            raise ValueError(f"unexpected parameter {key} {shape}")
    return sd
