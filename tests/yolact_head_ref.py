"""A torch restatement of the reference YOLACT neck and head — FeaturePyramid
(feature_pyramid.py:32-58), PredictionHead (prediction_head.py:90-143, with torchvision's
Bottleneck: conv1-bn1-relu, conv2-bn2-relu, conv3-bn3, + x, relu), Masknet (masknet.py:44-55) and the
concatenation of Yolact.forward (model.py:34-60) — as functions of a reference-layout state_dict.
BatchNorm in eval mode. tests/test_yolact_head_cpu.py pins it to the reference's goldens
(tests/golden/gen_golden_yolact_head.py); the GPU tests use it where no fixture exists (other
batch sizes, the per-level conv outputs behind the row order).
"""
import torch
import torch.nn.functional as F


def _conv(sd, p, x, stride=1, padding=0):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), stride=stride, padding=padding)


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                        training=False, eps=1e-5)


def _count(sd, prefix):
    n = 0
    while f"{prefix}.{n}.weight" in sd or f"{prefix}.{n}.conv1.weight" in sd:
        n += 1
    return n


def feature_pyramid(sd, maps, prefix="_feature_pyramid."):
    """-> the list of FPN levels [B, F, h, w]."""
    n = len(maps)
    lat = [_conv(sd, f"{prefix}_lateral_layers.{i}", maps[i]) for i in range(n)]
    pyr = [None] * n
    pyr[-1] = lat[-1]
    for i in range(n - 2, -1, -1):
        pyr[i] = lat[i] + F.interpolate(pyr[i + 1], lat[i].shape[2:4], mode="bilinear")
    out = [F.leaky_relu(_conv(sd, f"{prefix}_prediction_layers.{i}", pyr[i], padding=1)) for i in range(n)]
    for i in range(_count(sd, f"{prefix}_downsample_layers")):
        out.append(F.leaky_relu(_conv(sd, f"{prefix}_downsample_layers.{i}", out[-1], stride=2, padding=1)))
    return out


def _bottleneck(sd, p, x):
    y = F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x)))
    y = F.relu(_bn(sd, p + ".bn2", _conv(sd, p + ".conv2", y, padding=1)))
    y = _bn(sd, p + ".bn3", _conv(sd, p + ".conv3", y))
    return F.relu(y + x)


def _blocks(sd, prefix, group, x):
    for i in range(_count(sd, f"{prefix}{group}_layers")):
        x = F.relu(_conv(sd, f"{prefix}{group}_conv_layers.{i}", x) +
                   _bn(sd, f"{prefix}{group}_bn_layers.{i}", _bottleneck(sd, f"{prefix}{group}_layers.{i}", x)))
    return x


def prediction_head_raw(sd, x, prefix="_prediction_head."):
    """The three final convs' outputs [B, n_ar * width, h, w] of one level, before the
    permute / reshape / tanh."""
    x = _blocks(sd, prefix, "_extra", x)
    return (_conv(sd, prefix + "_classification_layer", _blocks(sd, prefix, "_classification_extra", x), padding=1),
            _conv(sd, prefix + "_box_encoding_layer", _blocks(sd, prefix, "_box_extra", x), padding=1),
            _conv(sd, prefix + "_mask_coeff_layer", _blocks(sd, prefix, "_mask_extra", x), padding=1))


def prediction_head(sd, x, n_classes, k, prefix="_prediction_head."):
    cls, box, coef = prediction_head_raw(sd, x, prefix)
    B = x.shape[0]
    return (cls.permute(0, 2, 3, 1).reshape(B, -1, n_classes + 1), box.permute(0, 2, 3, 1).reshape(B, -1, 4),
            torch.tanh(coef.permute(0, 2, 3, 1).reshape(B, -1, k)))


def masknet(sd, x, prefix="_masknet."):
    for i in (1, 2):
        x = F.leaky_relu(_conv(sd, f"{prefix}_layers_{i}.0.0", x, padding=1))
        x = F.leaky_relu(F.conv_transpose2d(x, sd[f"{prefix}_upsample_layer_{i}.weight"],
                                            sd[f"{prefix}_upsample_layer_{i}.bias"], stride=2, padding=1,
                                            output_padding=1))
    x = F.leaky_relu(_conv(sd, f"{prefix}_layers_3.0.0", x, padding=1))
    return F.leaky_relu(_conv(sd, prefix + "_output_layer", x))


def yolact_head(sd, maps, n_classes, k):
    """-> (classification [B, A, C+1], box_encoding [B, A, 4], mask_coeff [B, A, k], mask_prototype
    [B, k, 4h, 4w], the FPN levels): Yolact.forward without the backbone and the anchors."""
    fpn = feature_pyramid(sd, maps)
    proto = masknet(sd, fpn[0])
    parts = [prediction_head(sd, f, n_classes, k) for f in fpn]
    return (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1),
            torch.cat([p[2] for p in parts], 1), proto, fpn)
