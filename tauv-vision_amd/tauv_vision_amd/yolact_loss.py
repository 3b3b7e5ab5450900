"""The YOLACT training loss on the GPU — reference src/tauv_vision/yolact/model/loss.py:8-124, same name,
arguments and nested result, so that the swap in the reference's train.py is one import line:

    from tauv_vision_amd.yolact_loss import loss

`loss(prediction, truth, config) -> (total, (classification_loss, box_loss, mask_loss))` runs seven launches
(tv_yolact_loss_match / _select / _anchors / _mask_sums / _mask / _mask_coeff / _finalize,
csrc/yolact_loss.hip; six without gradients) whatever the batch size, the number of truths and the number
of positive anchors; the positive, negative and selected counts never come to the host. It is
differentiable with respect to classification, box_encoding, mask_coeff and mask_prototype through one
torch.autograd.Function: the forward launches write every tensor's unscaled gradient, and the backward
only multiplies each in place by (grad of total + grad of its own term) * the term's device-side factor,
so a graph can be walked back once. fp32 prediction tensors are taken as they are, with any strides;
nothing is copied. `loss_with_state` also returns the matching and mining sets.
"""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib

_GRADS = ("classification", "box_encoding", "mask_coeff", "mask_prototype")
_TERM_OF = (1, 2, 3, 3)  # the output value that is each gradient tensor's own term
_SEG_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)


def _as_u8(t):
    """A bool tensor's bytes as they are, anything else converted."""
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)


class _Call:
    """One loss call: the description the launches share, and the buffers they write."""

    def __init__(self, desc, keep, dev):
        self.desc, self.keep, self.dev, self.grads = desc, keep, dev, None

    def run(self, tensors, want_grad):
        d, dev = self.desc, self.dev
        self.grads = [torch.empty_like(t) for t in tensors] if want_grad else None
        for k, (n, t) in enumerate(zip(_GRADS, tensors)):
            setattr(d, n, t.data_ptr())
            getattr(d, n + "_stride")[:] = t.stride()
            if want_grad:
                setattr(d, "grad_" + n, self.grads[k].data_ptr())
                getattr(d, "grad_" + n + "_stride")[:] = self.grads[k].stride()
        lib, ref, s = _lib.lib(), ctypes.byref(d), _lib.stream_of(dev)
        n = ctypes.c_int64()
        _lib.check(lib.tv_yolact_loss_workspace_size(ref, ctypes.byref(n)), "yolact loss")
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        out = torch.empty(16, dtype=torch.float32, device=dev)
        wp = ctypes.c_void_p(ws.data_ptr())
        with torch.cuda.device(dev):
            for stage in _lib.YOLACT_LOSS_STAGES:
                if stage == "mask_coeff" and not want_grad:
                    continue
                _lib.check(getattr(lib, "tv_yolact_loss_" + stage)(ref, wp, n.value, s), "yolact loss")
            _lib.check(lib.tv_yolact_loss_finalize(ref, wp, n.value, ctypes.c_void_p(out.data_ptr()), s), "yolact loss")
        return out


class _YolactLoss(torch.autograd.Function):
    """(call, classification, box_encoding, mask_coeff, mask_prototype) -> the kernel's 16 output values."""

    @staticmethod
    def forward(ctx, call, *tensors):
        want = call.want_grad  # decided by loss_with_state(): inside forward() the grad mode is always off
        out = call.run(tensors, want)
        ctx.call = call if want else None
        if want:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        call = ctx.call
        if call is None or call.grads is None:
            raise RuntimeError("tauv_vision_amd.yolact_loss: the gradients of this loss call were already returned "
                               "(the backward pass scales them in place; call loss() again)")
        out, = ctx.saved_tensors
        scale = (g[0] + g[list(_TERM_OF)]) * out[8:12]
        grads, call.grads = call.grads, None
        lib, s = _lib.lib(), _lib.stream_of(call.dev)
        with torch.cuda.device(call.dev):
            for k, t in enumerate(grads):
                _lib.check(lib.tv_centernet_loss_scale(
                    ctypes.c_void_p(t.data_ptr()), _lib.DTYPES["fp32"], t.numel(),
                    ctypes.c_void_p(scale.data_ptr() + 4 * k), s), "yolact loss backward")
        return (None, *grads)


def loss_with_state(prediction, truth, config):
    """`loss` plus the record of the matching and the mining, device tensors [B, A]:
    -> (total, (classification_loss, box_loss, mask_loss), state) with state.match_index int32 (the matched
    truth index; meaningful at positives), state.positive, state.negative, state.selected uint8 (selected:
    the positives plus the mined negatives)."""
    classification, box_encoding, mask_coeff, anchor, mask_prototype = prediction
    truth_valid, truth_classification, truth_box, truth_seg_map, truth_img_valid = truth
    named = dict(zip(_GRADS + ("anchor",), (classification, box_encoding, mask_coeff, mask_prototype, anchor)))
    for n, t in named.items():
        if t.dtype != torch.float32:
            raise ValueError(f"yolact loss: {n} is {t.dtype}; the prediction must be fp32 (fp16 and bf16 are refused)")
    if classification.dim() != 3 or mask_prototype.dim() != 4:
        raise ValueError(f"yolact loss: classification must be [B, A, C] and mask_prototype [B, P, h, w], got "
                         f"{list(classification.shape)} and {list(mask_prototype.shape)}")
    B, A, C = classification.shape
    P, h, w = mask_prototype.shape[1:]
    want = {"box_encoding": (B, A, 4), "mask_coeff": (B, A, P), "anchor": (1, A, 4), "mask_prototype": (B, P, h, w)}
    for n, shape in want.items():
        if tuple(named[n].shape) != shape:
            raise ValueError(f"yolact loss: {n} is {list(named[n].shape)}, expected {list(shape)} "
                             f"(B, A, C = {B}, {A}, {C} from classification, P, h, w from mask_prototype)")
    if min(B, A, C, P, h, w) < 1:
        raise ValueError(f"yolact loss: empty prediction (B, A, C, P, h, w = {B}, {A}, {C}, {P}, {h}, {w})")
    if truth_valid.dim() != 2 or truth_valid.shape[0] != B:
        raise ValueError(f"yolact loss: truth_valid is {list(truth_valid.shape)} for a batch of {B}")
    T = truth_valid.shape[1]
    if T == 0:
        raise ValueError("yolact loss: T == 0 (the reference's max over no truth raises)")
    if tuple(truth_classification.shape) != (B, T) or tuple(truth_box.shape) != (B, T, 4):
        raise ValueError(f"yolact loss: truth_classification is {list(truth_classification.shape)} and truth_box "
                         f"{list(truth_box.shape)}, expected {[B, T]} and {[B, T, 4]}")
    if truth_seg_map.dim() != 3 or truth_seg_map.shape[0] != B or truth_seg_map.shape != truth_img_valid.shape \
            or truth_seg_map.numel() == 0:
        raise ValueError(f"yolact loss: truth_seg_map is {list(truth_seg_map.shape)} and truth_img_valid "
                         f"{list(truth_img_valid.shape)}, expected two non-empty [B, in_h, in_w] of a batch of {B}")
    if truth_seg_map.dtype not in _SEG_DTYPES or truth_classification.dtype.is_floating_point:
        raise ValueError(f"yolact loss: truth_seg_map is {truth_seg_map.dtype} and truth_classification "
                         f"{truth_classification.dtype}; both must be integers (uint8, int16, int32 or int64)")
    ratio = config.negative_example_ratio
    if ratio < 0 or int(ratio) != ratio:
        raise ValueError(f"yolact loss: negative_example_ratio must be an integer >= 0, got {ratio}")
    for n, t in named.items():
        if not t.is_cuda:
            raise ValueError(f"yolact loss: {n} is on the host; the loss runs on the GPU that holds the prediction")
        if t.device != classification.device:
            raise ValueError(f"yolact loss: {n} is on {t.device}, classification on {classification.device}")

    dev = classification.device
    keep = {"truth_valid": truth_valid.to(device=dev, dtype=torch.uint8).contiguous(),
            "truth_classification": truth_classification.to(device=dev, dtype=torch.int64).contiguous(),
            "truth_box": truth_box.to(device=dev, dtype=torch.float32).contiguous(),
            "truth_seg_map": truth_seg_map.to(dev).contiguous(),
            "truth_img_valid": _as_u8(truth_img_valid.to(dev)),
            "anchor": anchor}
    # F.cross_entropy raises on a class outside [0, C): the call's one device-to-host check
    tc = keep["truth_classification"]
    if bool(((tc < 0) | (tc >= C))[keep["truth_valid"].bool()].any()):
        raise IndexError(f"yolact loss: truth_classification out of range for {C} classes")
    state = SimpleNamespace(match_index=torch.empty((B, A), dtype=torch.int32, device=dev),
                            positive=torch.empty((B, A), dtype=torch.uint8, device=dev),
                            negative=torch.empty((B, A), dtype=torch.uint8, device=dev),
                            selected=torch.empty((B, A), dtype=torch.uint8, device=dev))

    d = _lib.YolactLossDesc()
    d.B, d.A, d.C, d.P, d.T, d.h, d.w = B, A, C, P, T, h, w
    d.in_h, d.in_w = truth_seg_map.shape[1:]
    d.seg_itemsize = keep["truth_seg_map"].element_size()
    d.negative_example_ratio = int(ratio)
    d.iou_pos_threshold, d.iou_neg_threshold = float(config.iou_pos_threshold), float(config.iou_neg_threshold)
    d.box_variances[:] = [float(config.box_variances[0]), float(config.box_variances[1])]
    d.anchor = anchor.data_ptr()
    d.anchor_stride[:] = anchor.stride()[1:]
    for n in ("truth_valid", "truth_classification", "truth_box", "truth_seg_map", "truth_img_valid"):
        setattr(d, n, keep[n].data_ptr())
    for n, t in vars(state).items():
        setattr(d, n, t.data_ptr())
    call = _Call(d, keep, dev)
    tensors = [named[n] for n in _GRADS]
    call.want_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    out = _YolactLoss.apply(call, *tensors)
    return out[0], (out[1], out[2], out[3]), state


def loss(prediction, truth, config):
    """loss.py:8-124 on the GPU.

    prediction = (classification [B, A, C], box_encoding [B, A, 4], mask_coeff [B, A, P], anchor [1, A, 4],
    mask_prototype [B, P, h, w]), fp32 on one GPU, any strides; truth = (truth_valid [B, T] bool,
    truth_classification [B, T] int, truth_box [B, T, 4], truth_seg_map [B, in_h, in_w] int,
    truth_img_valid [B, in_h, in_w] bool), on the host or the device (uint8 classes and seg maps go in as they
    are); config is read for iou_pos_threshold, iou_neg_threshold, negative_example_ratio and box_variances.
    -> (total, (classification_loss, box_loss, mask_loss)): fp32 device scalars. total.backward() and each
    term's own backward reach classification, box_encoding, mask_coeff and mask_prototype; the anchor and the
    truth carry no gradient. A second backward through the same call raises.

    Departure from the reference: with k = negative_example_ratio * n_positive larger than a sample's
    number of negatives, the reference's topk goes on into its -inf entries, the neutral and positive
    anchors, in an order torch does not define, and raises for k > A. Here min(k, n_negative) negatives
    are mined: every negative and nothing else. The denominator stays (1 + ratio) * sum n_positive.

    The reference's quirks, kept:
      * the truth mask is (truth_seg_map == match_index): the seg map is compared with the truth's index in
        the sample, not with its class;
      * a positive whose resized truth mask sums to exactly 0 adds nothing to the mask term but still counts
        in the batch's positive count, which divides the term;
      * without any positive the three terms are plain sums, which are 0.

    Refused before any launch (ValueError): prediction tensors on the host, not fp32 (fp16 and bf16 are
    out of scope), or of shapes that disagree (A, B, P); T == 0, where the reference's torch.max over an
    empty dimension raises; negative_example_ratio < 0. A truth_classification outside [0, C) at a valid
    truth raises IndexError, through the call's one small device-to-host check."""
    total, terms, _ = loss_with_state(prediction, truth, config)
    return total, terms
