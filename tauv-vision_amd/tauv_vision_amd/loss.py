"""The CenterNet training loss and its targets on the GPU — reference
src/tauv_vision/centernet/model/loss.py, same names, argument meaning and output layout.

Targets (loss.py:31-135): generate_heatmap, generate_keypoint_heatmap, out_index_for_position, backed by
tv_train_heatmap / tv_train_keypoint_targets (csrc/targets.hip).

Loss (loss.py:178-390): `loss(prediction, truth, model_config, train_config, object_config, img) -> Losses`
drops into the reference's train.py and run_validation_epoch. It runs three launches
(tv_centernet_loss_dense / _objects / _finalize, csrc/loss.hip) whatever the batch and object counts, stores
no target plane, and is differentiable with respect to every prediction tensor through one
torch.autograd.Function whose backward only scales the gradients the forward launches already wrote.
Prediction tensors are taken as they are (fp32 / fp16 / bf16, any strides: the reference model's
NCHW heatmaps and permuted heads, or this package's channel slices of one NHWC tensor); nothing is
copied. The helpers focal_loss, angle_loss, depth_loss, angle_range and angle_in_range keep the
reference's elementwise meaning and are plain torch expressions on their arguments' device, like
out_index_for_position: `loss` does not go through them.

`truth` is the reference's PoseSample (datasets/load/pose_dataset.py:25-41) or this module's
PoseSample; its tensors may be on the host (they are moved to the GPU). The targets are fp32 device
tensors.
"""
import ctypes
from dataclasses import dataclass
from enum import Enum
from math import pi
from typing import Optional

import torch

from . import _lib


@dataclass
class PoseSample:
    """The fields of the reference's PoseSample (pose_dataset.py:25-41) the targets and the loss read."""
    valid: torch.Tensor                           # [B, n_objects] bool
    label: torch.Tensor                           # [B, n_objects] int
    center: torch.Tensor                          # [B, n_objects, 2] (y, x) normalised
    keypoint_valid: Optional[torch.Tensor] = None         # [B, n_keypoint_instances] bool
    keypoint_label: Optional[torch.Tensor] = None         # [B, n_keypoint_instances] int
    keypoint_center: Optional[torch.Tensor] = None        # [B, n_keypoint_instances, 2]
    keypoint_object_index: Optional[torch.Tensor] = None  # [B, n_keypoint_instances] int
    img: Optional[torch.Tensor] = None
    size: Optional[torch.Tensor] = None                   # [B, n_objects, 2] normalised
    roll: Optional[torch.Tensor] = None                   # [B, n_objects] radians
    pitch: Optional[torch.Tensor] = None
    yaw: Optional[torch.Tensor] = None
    depth: Optional[torch.Tensor] = None                  # [B, n_objects]


def _as(t, dtype, dev):
    return t.to(device=dev, dtype=dtype).contiguous()


def _check_index(idx, valid, bound, what):
    """The reference indexes with these values (heatmap[sample_i, label]): out of range raises."""
    if idx.numel() and bool(((idx < -bound) | (idx >= bound))[valid].any()):
        raise IndexError(f"{what} out of range for {bound} planes")


def _out_shape(model_config):
    """The kernels derive the target grid as in_h // downsample_ratio x in_w // downsample_ratio
    (the reference ModelConfig's out_h / out_w, config.py:24-30) and write it through raw pointers:
    a duck-typed config whose out_h / out_w disagree would be written out of bounds."""
    r = int(model_config.downsample_ratio)
    if r < 1:
        raise ValueError(f"downsample_ratio must be >= 1, got {r}")
    H, W = int(model_config.in_h) // r, int(model_config.in_w) // r
    if (int(model_config.out_h), int(model_config.out_w)) != (H, W):
        raise ValueError(f"model_config.out_h/out_w = ({model_config.out_h}, {model_config.out_w}) but the "
                         f"targets grid is in_h // downsample_ratio x in_w // downsample_ratio = ({H}, {W})")
    return H, W


def generate_heatmap(truth, model_config, train_config, object_config) -> torch.Tensor:
    """loss.py:31-72 -> [B, n_labels, out_h, out_w] fp32 on the GPU."""
    H, W = _out_shape(model_config)
    dev = _lib.current_cuda(truth.valid)
    B, n_obj = truth.valid.shape
    L = object_config.n_labels
    valid = _as(truth.valid, torch.uint8, dev)
    label = _as(truth.label, torch.int64, dev)
    center = _as(truth.center, torch.float32, dev)
    _check_index(label, valid.bool(), L, "label")
    label = torch.where(label < 0, label + L, label)
    out = torch.empty((B, L, H, W), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().tv_train_heatmap(
        ctypes.c_void_p(valid.data_ptr()), ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(center.data_ptr()),
        B, n_obj, L, model_config.in_h, model_config.in_w, model_config.downsample_ratio,
        float(train_config.keypoint_heatmap_sigma), ctypes.c_void_p(out.data_ptr()), _lib.stream_of(dev)),
        "generate_heatmap")
    return out


def generate_keypoint_heatmap(truth, model_config, train_config, object_config):
    """loss.py:75-135 -> (heatmap, affinity_weight [B, n_keypoints, out_h, out_w],
    affinity [B, n_keypoints, 2, out_h, out_w]) fp32 on the GPU."""
    H, W = _out_shape(model_config)
    dev = _lib.current_cuda(truth.keypoint_valid)
    B, n_inst = truth.keypoint_valid.shape
    n_obj = truth.center.shape[1]
    K = object_config.n_keypoints
    kvalid = _as(truth.keypoint_valid, torch.uint8, dev)
    klabel = _as(truth.keypoint_label, torch.int64, dev)
    kcenter = _as(truth.keypoint_center, torch.float32, dev)
    kobj = _as(truth.keypoint_object_index, torch.int64, dev)
    center = _as(truth.center, torch.float32, dev)
    _check_index(klabel, kvalid.bool(), K, "keypoint_label")
    _check_index(kobj, kvalid.bool(), n_obj, "keypoint_object_index")
    klabel = torch.where(klabel < 0, klabel + K, klabel)
    kobj = torch.where(kobj < 0, kobj + n_obj, kobj)
    heat = torch.empty((B, K, H, W), dtype=torch.float32, device=dev)
    aw = torch.empty_like(heat)
    aff = torch.empty((B, K, 2, H, W), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().tv_train_keypoint_targets(
        ctypes.c_void_p(kvalid.data_ptr()), ctypes.c_void_p(klabel.data_ptr()), ctypes.c_void_p(kcenter.data_ptr()),
        ctypes.c_void_p(kobj.data_ptr()), ctypes.c_void_p(center.data_ptr()), B, n_inst, n_obj, K,
        model_config.in_h, model_config.in_w, model_config.downsample_ratio,
        float(train_config.keypoint_heatmap_sigma), float(train_config.keypoint_affinity_sigma),
        ctypes.c_void_p(heat.data_ptr()), ctypes.c_void_p(aw.data_ptr()), ctypes.c_void_p(aff.data_ptr()),
        _lib.stream_of(dev)), "generate_keypoint_heatmap")
    return heat, aw, aff


def out_index_for_position(position: torch.Tensor, model_config) -> torch.Tensor:
    """loss.py:131-135: output cell (y, x) of normalised positions [B, n, 2] (a two-op
    elementwise map, left to torch on the positions' device)."""
    return torch.stack((
        torch.clamp(((position[:, :, 0] * model_config.in_h) / model_config.downsample_ratio).to(torch.long), 0,
                    model_config.out_h - 1),
        torch.clamp(((position[:, :, 1] * model_config.in_w) / model_config.downsample_ratio).to(torch.long), 0,
                    model_config.out_w - 1),
    ), dim=-1)


@dataclass
class Losses:
    """loss.py:14-28. `heatmap` is the same tensor as `total` (see `loss`)."""
    total: torch.Tensor = torch.zeros(1)
    heatmap: torch.Tensor = torch.zeros(1)
    keypoint_heatmap: torch.Tensor = torch.zeros(1)
    keypoint_affinity: torch.Tensor = torch.zeros(1)
    offset: torch.Tensor = torch.zeros(1)
    size: torch.Tensor = torch.zeros(1)
    roll: torch.Tensor = torch.zeros(1)
    pitch: torch.Tensor = torch.zeros(1)
    yaw: torch.Tensor = torch.zeros(1)
    depth: torch.Tensor = torch.zeros(1)

    avg_size_error: torch.Tensor = torch.zeros(1)
    max_size_error: torch.Tensor = torch.zeros(1)


class Angle(Enum):
    Roll = 0
    Pitch = 1
    Yaw = 2


def _moduli(object_config, angle: Angle):
    axis = ("roll", "pitch", "yaw")[angle.value]
    return [0.0 if getattr(c, axis).modulo is None else float(getattr(c, axis).modulo) for c in object_config.configs]


def angle_range(truth_label: torch.Tensor, object_config, angle: Angle) -> torch.Tensor:
    """loss.py:151-175: the modulo of `angle` of each object's label, [B, n_objects] fp32 on the labels'
    device; 0 where the label has none (a table lookup instead of the reference's Python loop)."""
    table = torch.tensor(_moduli(object_config, angle), dtype=torch.float32, device=truth_label.device)
    return table[truth_label.long()]


def angle_in_range(angles: torch.Tensor, range_min: float, range_max: float) -> torch.Tensor:
    """loss.py:320-331: whether each angle lies in [range_min, range_max] modulo 2 pi."""
    range_min = range_min % (2 * pi)
    range_max = range_max % (2 * pi)
    angles = angles % (2 * pi)
    if range_min < range_max:
        return (range_min <= angles) & (angles <= range_max)
    return (range_min <= angles) | (angles <= range_max)


def focal_loss(prediction: torch.Tensor, truth: torch.Tensor, alpha: float, beta: float) -> torch.Tensor:
    """loss.py:302-317, elementwise: `prediction` holds probabilities (after the sigmoid), `truth` a
    target plane of the same shape. focal_loss(sigmoid(prediction.heatmap), generate_heatmap(...), a, b)
    .sum() is the heatmap term alone."""
    p = torch.isclose(truth, torch.ones((), dtype=truth.dtype, device=truth.device))
    N = torch.sum(p)
    pf = p.float()
    loss_p = ((1 - prediction) ** alpha) * torch.log(torch.clamp(prediction, min=1e-4)) * pf
    loss_n = ((1 - truth) ** beta) * (prediction ** alpha) * torch.log(torch.clamp(1 - prediction, min=1e-4)) * (1 - pf)
    return torch.where(N == 0, -loss_p, -(loss_p + loss_n) / N)


def angle_loss(predicted_bin: torch.Tensor, predicted_offset: torch.Tensor, truth: torch.Tensor,
               theta_range: torch.Tensor, bin_overlap: float) -> torch.Tensor:
    """loss.py:334-376: predicted_bin / predicted_offset [B, n, 4] ([outside, inside] logits and
    [sin, cos] offsets of bin 0, then bin 1), truth / theta_range [B, n] -> [B, n]."""
    from .decode import angle_get_bins
    import torch.nn.functional as F
    B, n = truth.shape
    truth = truth % theta_range
    truth = truth * (2 * pi / theta_range)
    (c0, lo0, hi0), (c1, lo1, hi1) = angle_get_bins(bin_overlap)
    result = 0
    for k, (c, lo, hi) in enumerate(((c0, lo0, hi0), (c1, lo1, hi1))):
        inside = angle_in_range(truth, lo, hi).to(torch.long).reshape(-1)
        target = torch.stack((torch.sin(truth - c), torch.cos(truth - c)), dim=-1).reshape(-1, 2)
        cls = F.cross_entropy(predicted_bin[:, :, 2 * k:2 * k + 2].reshape(-1, 2), inside, reduction="none")
        off = F.l1_loss(predicted_offset[:, :, 2 * k:2 * k + 2].reshape(-1, 2), target, reduction="none").sum(dim=-1)
        result = result + cls + inside.to(torch.float) * off
    return result.reshape(B, n)


def depth_loss(prediction: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """loss.py:379-390: |1 / sigmoid(prediction) - 1 - truth|, [B, n]."""
    return (1 / torch.sigmoid(prediction.reshape(-1)) - 1 - truth.reshape(-1)).abs().reshape(truth.shape)


# which of the kernel's output values (tv_centernet_loss_finalize) is the term of prediction tensor i
_TERM_OF_TENSOR = (11, 1, 2, 4, 3, 5, 5, 6, 6, 7, 7, 8)
_DTYPES = {torch.float32: _lib.DTYPES["fp32"], torch.float16: _lib.DTYPES["fp16"], torch.bfloat16: _lib.DTYPES["bf16"]}
_range_tables = {}


def _range_table(object_config, dev):
    """[3, n_labels] fp32 on `dev`: the roll, pitch, yaw modulo per label, uploaded once per table."""
    key = (tuple(_moduli(object_config, Angle.Roll)), tuple(_moduli(object_config, Angle.Pitch)),
           tuple(_moduli(object_config, Angle.Yaw)), dev)
    t = _range_tables.get(key)
    if t is None:
        t = _range_tables[key] = torch.tensor(key[:3], dtype=torch.float32, device=dev)
    return t


class _Call:
    """One loss call: the description the three launches share, and the buffers they write."""

    def __init__(self, desc, keep, dev, present):
        self.desc, self.keep, self.dev, self.present = desc, keep, dev, present

    def run(self, tensors, want_grad):
        d, dev = self.desc, self.dev
        self.grads = [torch.empty_like(t) for t in tensors] if want_grad else None
        for k, (i, t) in enumerate(zip(self.present, tensors)):
            e = d.tensor[i]
            e.data = t.data_ptr()
            e.stride[:t.dim()] = t.stride()
            if want_grad:
                e.grad = self.grads[k].data_ptr()
                e.grad_stride[:t.dim()] = self.grads[k].stride()
        lib, ref, s = _lib.lib(), ctypes.byref(d), _lib.stream_of(dev)
        n = ctypes.c_int64()
        _lib.check(lib.tv_centernet_loss_workspace_size(ref, ctypes.byref(n)), "loss")
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        out = torch.empty(32, dtype=torch.float32, device=dev)
        wp = ctypes.c_void_p(ws.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(lib.tv_centernet_loss_dense(ref, wp, n.value, s), "loss")
            _lib.check(lib.tv_centernet_loss_objects(ref, wp, n.value, s), "loss")
            _lib.check(lib.tv_centernet_loss_finalize(ref, wp, n.value, ctypes.c_void_p(out.data_ptr()), s), "loss")
        return out


class _CenternetLoss(torch.autograd.Function):
    """(call, *present prediction tensors) -> the kernel's 32 output values (values 0..11 are the terms).
    The forward writes every tensor's unscaled gradient; the backward multiplies it in place by
    (grad of total + grad of the tensor's own term) * the term's device-side factor and returns it, so a
    graph can be walked back once."""

    @staticmethod
    def forward(ctx, call, *tensors):
        want = call.want_grad  # decided by loss(): inside forward() the grad mode is always off
        out = call.run(tensors, want)
        ctx.call = call if want else None
        if want:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        call = ctx.call
        if call is None or call.grads is None:
            raise RuntimeError("tauv_vision_amd.loss: the gradients of this loss call were already returned "
                               "(the backward pass scales them in place; call loss() again)")
        out, = ctx.saved_tensors
        idx = [_TERM_OF_TENSOR[i] for i in call.present]
        scale = (g[0] + g[idx]) * out[16:28][list(call.present)]
        grads, call.grads = call.grads, None
        # (a half tensor's mul_ by a 0-dim fp32 tensor would round the scalar to half first)
        lib, s = _lib.lib(), _lib.stream_of(call.dev)
        with torch.cuda.device(call.dev):
            for k, t in enumerate(grads):
                _lib.check(lib.tv_centernet_loss_scale(
                    ctypes.c_void_p(t.data_ptr()), _DTYPES[t.dtype], t.numel(),
                    ctypes.c_void_p(scale.data_ptr() + 4 * k), s), "loss backward")
        return (None, *grads)


def loss(prediction, truth, model_config, train_config, object_config, img=None) -> Losses:
    """loss.py:178-299 on the GPU: the focal heatmap and keypoint-heatmap terms, the weighted affinity MSE,
    the size / offset L1, angle_loss per trained angle and depth_loss, with the reference's lambdas, in
    three launches. Heads that are None in `prediction` are skipped. The returned values are fp32 device
    scalars; `total.backward()` reaches every prediction tensor. avg_size_error / max_size_error carry no
    gradient.

    The reference's quirks, kept:
      * n_valid = min(int(valid.sum()), 1): the size, offset, angle and depth sums are divided by 1, not by
        the object count, and with no valid object they are 0 / 0 = NaN, and so is `total`;
      * angle_loss(...).sum() runs over all objects, invalid ones included, and is then multiplied by the
        valid count and divided by n_valid: gradients reach invalid objects' cells too;
      * `l = l_heatmap; l += ...` adds in place, so `losses.heatmap` is the same tensor as `losses.total`
        (the heatmap term alone: focal_loss(sigmoid(prediction.heatmap), generate_heatmap(...)).sum());
      * `truth % theta_range` is torch.remainder: a label whose angle has `modulo` None gives range 0 and a
        NaN term;
      * the `sigma < 0.1` clamp applies to the object heatmap only (generate_heatmap), not to the keypoint
        heatmap, although both use keypoint_heatmap_sigma.

    Refused before any launch (ValueError): prediction tensors on the host, of mixed or unsupported dtypes
    or of shapes that disagree with the config; a head present in `prediction` whose field is missing from
    `truth`. Labels and keypoint indices are validated like the target generators do, in the call's one
    device-to-host copy (IndexError); the valid count never comes to the host."""
    H, W = _out_shape(model_config)
    pred = {n: getattr(prediction, n, None) for n in _lib.LOSS_TENSORS}
    heat = pred["heatmap"]
    for n in ("heatmap", "size", "offset"):
        if pred[n] is None:
            raise ValueError(f"loss: prediction.{n} is required")
    B = heat.shape[0] if heat.dim() == 4 else -1
    L, K = int(object_config.n_labels), int(object_config.n_keypoints)
    want_shape = {"heatmap": (B, L, H, W), "keypoint_heatmap": (B, K, H, W), "keypoint_affinity": (B, K, 2, H, W),
                  "size": (B, H, W, 2), "offset": (B, H, W, 2), "depth": (B, H, W, 1)}
    present = tuple(i for i, n in enumerate(_lib.LOSS_TENSORS) if pred[n] is not None)
    for i in present:
        n, t = _lib.LOSS_TENSORS[i], pred[_lib.LOSS_TENSORS[i]]
        if not t.is_cuda:
            raise ValueError(f"loss: prediction.{n} is on the host; the loss runs on the GPU that holds the prediction")
        if t.device != heat.device or t.dtype != heat.dtype or t.dtype not in _DTYPES:
            raise ValueError(f"loss: prediction.{n} is {t.dtype} on {t.device}; every head must be fp32, fp16 or bf16, "
                             f"all alike, on {heat.device}")
        if tuple(t.shape) != want_shape.get(n, (B, H, W, 4)) or B < 1:
            raise ValueError(f"loss: prediction.{n} is {list(t.shape)}, the config gives "
                             f"{list(want_shape.get(n, (B, H, W, 4)))}")
    if pred["keypoint_affinity"] is not None and pred["keypoint_heatmap"] is None:
        raise ValueError("loss: prediction.keypoint_affinity needs prediction.keypoint_heatmap")
    angles = [a for a in ("roll", "pitch", "yaw") if pred[a + "_bin"] is not None or pred[a + "_offset"] is not None]
    for a in angles:
        if pred[a + "_bin"] is None or pred[a + "_offset"] is None:
            raise ValueError(f"loss: prediction.{a}_bin and prediction.{a}_offset go together")
    needed = ["valid", "label", "center", "size"] + angles + (["depth"] if pred["depth"] is not None else [])
    if pred["keypoint_heatmap"] is not None:
        needed += ["keypoint_valid", "keypoint_label", "keypoint_center", "keypoint_object_index"]
    for f in needed:
        if getattr(truth, f, None) is None:
            raise ValueError(f"loss: the prediction has a head that needs truth.{f}, which is missing")
    dev = heat.device
    n_obj = truth.valid.shape[1]
    if tuple(truth.valid.shape) != (B, n_obj):
        raise ValueError(f"loss: truth.valid is {list(truth.valid.shape)} for a batch of {B}")

    keep = {"valid": _as(truth.valid, torch.uint8, dev), "label": _as(truth.label, torch.int64, dev)}
    for f in ["center", "size"] + angles + (["depth"] if pred["depth"] is not None else []):
        keep[f] = _as(getattr(truth, f), torch.float32, dev)
    want_numel = {"valid": B * n_obj, "label": B * n_obj, "center": 2 * B * n_obj, "size": 2 * B * n_obj}
    idx, ok, bound = [keep["label"].reshape(-1)], [], [torch.full((B * n_obj,), L, device=dev)]
    # the reference's angle_range indexes the config list with every object's label, valid or not
    ok.append(torch.ones(B * n_obj, dtype=torch.bool, device=dev) if angles else keep["valid"].reshape(-1).bool())
    n_inst = 0
    if pred["keypoint_heatmap"] is not None:
        n_inst = truth.keypoint_valid.shape[1]
        keep["keypoint_valid"] = _as(truth.keypoint_valid, torch.uint8, dev)
        keep["keypoint_label"] = _as(truth.keypoint_label, torch.int64, dev)
        keep["keypoint_object_index"] = _as(truth.keypoint_object_index, torch.int64, dev)
        keep["keypoint_center"] = _as(truth.keypoint_center, torch.float32, dev)
        want_numel.update(keypoint_valid=B * n_inst, keypoint_label=B * n_inst, keypoint_object_index=B * n_inst,
                          keypoint_center=2 * B * n_inst)
        kv = keep["keypoint_valid"].reshape(-1).bool()
        idx += [keep["keypoint_label"].reshape(-1), keep["keypoint_object_index"].reshape(-1)]
        ok += [kv, kv]
        bound += [torch.full((B * n_inst,), K, device=dev), torch.full((B * n_inst,), n_obj, device=dev)]
    for f in angles + (["depth"] if pred["depth"] is not None else []):
        want_numel[f] = B * n_obj
    for f, n in want_numel.items():
        if keep[f].numel() != n:
            raise ValueError(f"loss: truth.{f} has {keep[f].numel()} elements, expected {n}")
    _check_index(torch.cat(idx), torch.cat(ok), torch.cat(bound), "label / keypoint_label / keypoint_object_index")
    keep["label"] = torch.where(keep["label"] < 0, keep["label"] + L, keep["label"])
    if n_inst:
        for f, m in (("keypoint_label", K), ("keypoint_object_index", n_obj)):
            keep[f] = torch.where(keep[f] < 0, keep[f] + m, keep[f])
    if angles:
        keep["angle_range"] = _range_table(object_config, dev)

    d = _lib.LossDesc()
    d.dtype, d.B, d.n_objects, d.n_instances, d.n_labels, d.n_keypoints = _DTYPES[heat.dtype], B, n_obj, n_inst, L, K
    d.in_h, d.in_w, d.downsample_ratio = int(model_config.in_h), int(model_config.in_w), \
        int(model_config.downsample_ratio)
    d.keypoint_heatmap_sigma = float(train_config.keypoint_heatmap_sigma)
    d.keypoint_affinity_sigma = float(getattr(train_config, "keypoint_affinity_sigma", 1.0))
    d.focal_alpha, d.focal_beta = float(train_config.heatmap_focal_loss_a), float(train_config.heatmap_focal_loss_b)
    for f in ("keypoint_heatmap", "keypoint_affinity", "size", "offset", "angle", "depth"):
        setattr(d, "lambda_" + f, float(getattr(train_config, "loss_lambda_" + f, 0.0)))
    if angles:
        from .decode import angle_get_bins
        for k, b in enumerate(angle_get_bins(model_config.angle_bin_overlap)):
            d.bins[k][:] = [float(v) for v in b]
    for f, t in keep.items():
        setattr(d, f, t.data_ptr() if t.numel() else None)
    call, tensors = _Call(d, keep, dev, present), [pred[_lib.LOSS_TENSORS[i]] for i in present]
    call.want_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    out = _CenternetLoss.apply(call, *tensors)

    losses = Losses()
    losses.total = losses.heatmap = out[0]
    for k, f in ((1, "keypoint_heatmap"), (2, "keypoint_affinity")):
        if pred[f] is not None:
            setattr(losses, f, out[k])
    losses.offset, losses.size = out[3], out[4]
    for k, a in ((5, "roll"), (6, "pitch"), (7, "yaw")):
        if a in angles:
            setattr(losses, a, out[k])
    if pred["depth"] is not None:
        losses.depth = out[8]
    losses.avg_size_error, losses.max_size_error = out[9].detach(), out[10].detach()
    return losses
