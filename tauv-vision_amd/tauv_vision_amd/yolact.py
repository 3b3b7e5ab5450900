"""Drop-in YOLACT protonet and post-processing (reference
src/tauv_vision/yolact/model/): `Masknet` (masknet.py:8-55), `get_anchor` (anchors.py:9-41),
`box_encode` / `box_decode` (boxes.py:45-61), `nms` (nms.py:7-29) and `assemble_mask`
(masks.py:8-21), as called by the YOLACT node (yolact_node.py:118-134), plus batched forms of
nms / assemble_mask for B images at once.

Masknet, box_encode/decode, nms and assemble_mask run in the HIP library (csrc/) on the tensors'
GPU; there is no CPU fallback. `get_anchor` builds the per-level anchor constants on the host
exactly like the reference (it is configuration, computed once per FPN level).
"""
from dataclasses import dataclass
from math import sqrt
from typing import NamedTuple, Optional, Tuple

import ctypes
import torch
import torch.nn as nn

from . import _lib
from .dla import populate
from .engine import NativeEngine
from .native import NativeModule
from .weights import model_io, param_layout, protonet_desc, resnet18_desc, yolact_desc, yolact_head_desc


@dataclass
class YolactConfig:
    """The fields of the reference yolact ModelConfig (config.py:8-40) the protonet and the
    post-processing read."""
    in_w: int
    in_h: int
    anchor_scales: Tuple[int, ...]
    anchor_aspect_ratios: Tuple[float, ...]
    box_variances: Tuple[float, float]
    feature_depth: int = 256
    n_prototype_masks: int = 8
    # read by the neck and the head (FeaturePyramid, PredictionHead, YolactHead)
    n_classes: int = 1
    n_prediction_head_layers: int = 1
    n_classification_layers: int = 0
    n_box_layers: int = 0
    n_mask_layers: int = 0
    n_fpn_downsample_layers: int = 2
    # the node's T.Normalize (yolact_node.py:111). The kernels hold the ImageNet constants every
    # reference config uses: forward_frames / detect refuse any other value
    img_mean: Tuple[float, float, float] = (0.485, 0.456, 0.406)
    img_stddev: Tuple[float, float, float] = (0.229, 0.224, 0.225)


IMAGENET_MEAN, IMAGENET_STDDEV = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _head_layers(config):
    return (int(config.n_prediction_head_layers), int(config.n_classification_layers), int(config.n_box_layers),
            int(config.n_mask_layers))


def _head_desc(in_depths, sizes, config, precision, fpn_only=False):
    return yolact_head_desc(in_depths, sizes, int(config.feature_depth), int(config.n_fpn_downsample_layers),
                            int(config.n_classes), int(config.n_prototype_masks), len(config.anchor_aspect_ratios),
                            _head_layers(config), precision, fpn_only)


class Masknet(NativeModule):
    """masknet.py:8-55: fpn[0] [B, F, H, W] -> prototypes [B, k, 4H, 4W] (LeakyReLU output).

    Parameters keep the reference key layout (`_layers_1.0.0.weight`, `_upsample_layer_1.weight`,
    ..., `_output_layer.bias`), so `load_state_dict` of a reference Masknet (or of the `_masknet.`
    sub-dict of a Yolact checkpoint) works unchanged. The forward pass is one native call: the
    3x3 convs as MFMA implicit GEMMs, each ConvTranspose2d(3, s2, p1) as four phase GEMMs (one per
    output parity, exactly its 9 taps per 2x2 block), bias + LeakyReLU in the epilogues. The result
    is a [B, k, 4H, 4W] view of one fp32 NHWC tensor (the layout assemble_mask reads fastest).
    `precision`: "fp32" (exact-f32 MFMA, parity mode), "fp16" or "bf16" (fp32 accumulation)."""

    def __init__(self, config, precision: str = "fp32"):
        super().__init__()
        self.feature_depth = int(config.feature_depth)
        self.n_prototype_masks = int(config.n_prototype_masks)
        self._init_native(precision)
        layout = param_layout(protonet_desc(self.feature_depth, self.n_prototype_masks))
        populate(self, layout, seed_layout=layout)

    def engine(self, device: torch.device, fpn_h: int, fpn_w: int) -> NativeEngine:
        return self._engine(device, (fpn_h, fpn_w),
                            lambda: protonet_desc(self.feature_depth, self.n_prototype_masks, fpn_h, fpn_w,
                                                  self.precision), self.state_dict)

    def forward_nhwc(self, fpn_output: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The native result: fp32 NHWC [B, 4H, 4W, k rounded up to 4]."""
        if fpn_output.dim() != 4 or fpn_output.shape[1] != self.feature_depth:
            raise ValueError(f"expected fpn_output [batch, {self.feature_depth}, H, W], got {tuple(fpn_output.shape)}")
        dev = _lib.current_cuda(fpn_output)
        x = fpn_output.to(dev, torch.float32).contiguous()
        return self.engine(dev, x.shape[2], x.shape[3]).forward(x, out)

    def forward(self, fpn_output: torch.Tensor) -> torch.Tensor:
        return self.forward_nhwc(fpn_output)[..., :self.n_prototype_masks].permute(0, 3, 1, 2)


def get_anchor(fpn_i: int, fpn_size, config) -> torch.Tensor:
    """anchors.py:9-41: [1, H*W*n_ar, 4] (y, x, h, w) at cell centres; per aspect ratio a block."""
    n = len(config.anchor_aspect_ratios)
    y = (torch.arange(0, fpn_size[0]) + 0.5) / fpn_size[0]
    x = (torch.arange(0, fpn_size[1]) + 0.5) / fpn_size[1]
    y, x = torch.meshgrid(y, x, indexing="ij")
    y = torch.tile(y.flatten(), (1, n))
    x = torch.tile(x.flatten(), (1, n))
    scale = config.anchor_scales[fpn_i]
    in_size = (config.in_h + config.in_w) / 2
    hw = fpn_size[0] * fpn_size[1]
    h = torch.cat([torch.full((1, hw), (scale / in_size) * sqrt(ar)) for ar in config.anchor_aspect_ratios], -1)
    w = torch.cat([torch.full((1, hw), (scale / in_size) / sqrt(ar)) for ar in config.anchor_aspect_ratios], -1)
    return torch.stack((y, x, h, w), dim=1).permute(0, 2, 1)


def _f32(t, name):
    return _lib.require_gpu_tensor(t, name).contiguous()


def _boxes_op(fn, name, a: torch.Tensor, anchor: torch.Tensor, config, out=None) -> torch.Tensor:
    x = _f32(a, name)
    anc = _f32(anchor, "anchor").to(x.device)
    if x.dim() != 3 or x.shape[-1] != 4 or anc.dim() != 3 or anc.shape[1:] != x.shape[1:]:
        raise ValueError(f"{name}: {tuple(x.shape)} / anchors {tuple(anc.shape)} mismatch")
    out = _lib.check_out(out, x.shape, x.device, name)
    B, A, _ = x.shape
    _lib.check(fn(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(anc.data_ptr()), B, A, anc.shape[0],
                  float(config.box_variances[0]), float(config.box_variances[1]), ctypes.c_void_p(out.data_ptr()),
                  _lib.stream_of(x.device)), name)
    return out


def box_decode(box_encoding: torch.Tensor, anchor: torch.Tensor, config, out=None) -> torch.Tensor:
    """boxes.py:55-61 on the GPU: [B, A, 4] encodings + [1 or B, A, 4] anchors -> boxes (y, x, h, w).
    `out`: a caller-owned contiguous fp32 [B, A, 4] buffer (no allocation per call)."""
    return _boxes_op(_lib.lib().tv_yolact_box_decode, "box_decode", box_encoding, anchor, config, out)


def box_encode(box: torch.Tensor, anchor: torch.Tensor, config) -> torch.Tensor:
    """boxes.py:45-53 on the GPU: [B, A, 4] boxes (y, x, h, w) + [1 or B, A, 4] anchors -> encodings."""
    return _boxes_op(_lib.lib().tv_yolact_box_encode, "box_encode", box, anchor, config)


def _nms_args(classification, box):
    cls = _f32(classification, "classification")
    bx = _f32(box, "box").to(cls.device)
    if cls.dim() != 3 or bx.dim() != 3 or bx.shape[-1] != 4 or cls.shape[1] != bx.shape[1]:
        raise ValueError(f"nms: classification {tuple(cls.shape)} / box {tuple(bx.shape)} mismatch")
    return cls, bx


def nms(classification: torch.Tensor, box: torch.Tensor, top_k: int, iou_threshold: float,
        confidence_threshold: float) -> torch.Tensor:
    """nms.py:7-29 (YOLACT fast NMS, batch 0 only): int64 indices of the kept anchors in
    descending-confidence order. Any anchor count. One device->host read of the kept count."""
    cls, bx = _nms_args(classification, box)
    A, C1 = cls.shape[1], cls.shape[2]
    K = min(int(top_k), A)
    det = torch.empty((max(K, 1),), dtype=torch.int64, device=cls.device)
    n = torch.empty((1,), dtype=torch.int32, device=cls.device)
    _lib.check(_lib.lib().tv_yolact_fast_nms(ctypes.c_void_p(cls[0].data_ptr()), A, C1, ctypes.c_void_p(bx[0].data_ptr()),
                                             int(top_k), float(iou_threshold), float(confidence_threshold),
                                             ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(n.data_ptr()),
                                             _lib.stream_of(cls.device)), "nms")
    return det[:int(n.item())]


class BatchedNMS:
    """nms.py:7-29 applied to every image of a [B, A, C+1] / [B, A, 4] batch with static device
    buffers (graph-capturable, no host sync): returns (det [B, min(top_k, A)] int64 — row b's first
    counts[b] entries are its kept anchors in descending confidence —, counts [B] int32)."""

    def __init__(self, B, A, top_k, device):
        self.B, self.A, self.top_k = int(B), int(A), int(top_k)
        self.K = min(self.top_k, self.A)
        nbytes = ctypes.c_int64()
        _lib.check(_lib.lib().tv_yolact_nms_workspace_size(self.B, self.A, self.top_k, ctypes.byref(nbytes)),
                   "nms workspace")
        self.ws = torch.empty((max(nbytes.value, 256),), dtype=torch.uint8, device=device)
        self.det = torch.zeros((self.B, self.K), dtype=torch.int64, device=device)
        self.counts = torch.zeros((self.B,), dtype=torch.int32, device=device)

    def __call__(self, classification, box, iou_threshold, confidence_threshold):
        cls, bx = _nms_args(classification, box)
        if cls.shape[0] != self.B or cls.shape[1] != self.A:
            raise ValueError(f"BatchedNMS built for [{self.B}, {self.A}], got {tuple(cls.shape)}")
        _lib.check(_lib.lib().tv_yolact_fast_nms_batched(
            ctypes.c_void_p(cls.data_ptr()), self.B, self.A, cls.shape[2], ctypes.c_void_p(bx.data_ptr()), self.top_k,
            float(iou_threshold), float(confidence_threshold), ctypes.c_void_p(self.det.data_ptr()),
            ctypes.c_void_p(self.counts.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(),
            _lib.stream_of(cls.device)), "nms_batched")
        return self.det, self.counts


def _proto_view(t, name):
    t = _lib.require_gpu_tensor(t, name)
    if t.stride()[-1] != 1 and t.stride()[-3] != 1:
        t = t.contiguous()
    return t


def assemble_mask(mask_prototype: torch.Tensor, mask_coeff: torch.Tensor,
                  box: Optional[torch.Tensor]) -> torch.Tensor:
    """masks.py:8-21: prototypes [K, H, W] (any strides: NCHW slices or Masknet's NHWC view),
    coefficients [n, K], boxes [n, 4] or None -> [n, H, W]."""
    proto = _proto_view(mask_prototype, "mask_prototype")
    coeff = _f32(mask_coeff, "mask_coeff").to(proto.device)
    if proto.dim() != 3 or coeff.dim() != 2 or coeff.shape[1] != proto.shape[0]:
        raise ValueError(f"assemble_mask: prototypes {tuple(proto.shape)} / coefficients {tuple(coeff.shape)} mismatch")
    bptr = None
    if box is not None:
        box = _f32(box, "box").to(proto.device)
        if box.shape != (coeff.shape[0], 4):
            raise ValueError(f"assemble_mask: box {tuple(box.shape)} must be [n, 4]")
        bptr = ctypes.c_void_p(box.data_ptr())
    K, H, W = proto.shape
    n = coeff.shape[0]
    out = torch.empty((n, H, W), dtype=torch.float32, device=proto.device)
    if n == 0:  # no detections (the node returns before this, yolact_node.py:131-133)
        return out
    _lib.check(_lib.lib().tv_yolact_assemble_mask(ctypes.c_void_p(proto.data_ptr()), _lib.strides(proto, 3), K, H, W,
                                                  ctypes.c_void_p(coeff.data_ptr()), bptr, n,
                                                  ctypes.c_void_p(out.data_ptr()), _lib.stream_of(proto.device)),
               "assemble_mask")
    return out


def _on(t, device, what):
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the prototypes on {device}")
    return t


def assemble_masks(mask_prototype: torch.Tensor, mask_coeff: torch.Tensor, box: Optional[torch.Tensor],
                   counts: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """assemble_mask for B images: prototypes [B, K, H, W] (any strides), coefficients
    [B, n, K], boxes [B, n, 4] or None, counts [B] int32 on the device (detections per image;
    None = all n) -> masks [B, n, H, W] (rows past counts[b] are left untouched)."""
    proto = _proto_view(mask_prototype, "mask_prototype")
    coeff = _on(_f32(mask_coeff, "mask_coeff"), proto.device, "mask_coeff")
    if proto.dim() != 4 or coeff.dim() != 3:
        raise ValueError(f"assemble_masks: prototypes {tuple(proto.shape)} / coefficients {tuple(coeff.shape)}")
    B, K, H, W = proto.shape
    n = coeff.shape[1]
    if coeff.shape != (B, n, K):
        raise ValueError(f"assemble_masks: coefficients {tuple(coeff.shape)} must be [{B}, n, {K}]")
    bptr = cptr = None
    if box is not None:
        box = _on(_f32(box, "box"), proto.device, "box")
        if box.shape != (B, n, 4):
            raise ValueError(f"assemble_masks: box {tuple(box.shape)} must be [{B}, {n}, 4]")
        bptr = ctypes.c_void_p(box.data_ptr())
    if counts is not None:
        if counts.dtype != torch.int32 or counts.shape != (B,) or counts.device != proto.device \
                or not counts.is_contiguous():
            raise ValueError("assemble_masks: counts must be a contiguous int32 [B] tensor on the prototypes' device")
        cptr = ctypes.c_void_p(counts.data_ptr())
    out = _lib.check_out(out, (B, n, H, W), proto.device, "assemble_masks")
    _lib.check(_lib.lib().tv_yolact_assemble_masks(ctypes.c_void_p(proto.data_ptr()), _lib.strides(proto, 4), B, K, H, W,
                                                   ctypes.c_void_p(coeff.data_ptr()), bptr, cptr, n,
                                                   ctypes.c_void_p(out.data_ptr()), _lib.stream_of(proto.device)),
               "assemble_masks")
    return out


def assemble_masks_indexed(mask_prototype: torch.Tensor, mask_coeff: torch.Tensor, box: Optional[torch.Tensor],
                           det: torch.Tensor, counts: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The node's mask step (yolact_node.py:134) for B images straight from BatchedNMS: prototypes
    [B, K, H, W] (any strides), coefficients [B, A, K] and boxes [B, A, 4] (or None) of every anchor,
    det [B, n] int64 / counts [B] int32 (BatchedNMS outputs) -> masks [B, n, H, W]; rows past
    counts[b] are left untouched."""
    proto = _proto_view(mask_prototype, "mask_prototype")
    coeff = _on(_f32(mask_coeff, "mask_coeff"), proto.device, "mask_coeff")
    if proto.dim() != 4 or coeff.dim() != 3 or det.dim() != 2:
        raise ValueError("assemble_masks_indexed: need prototypes [B, K, H, W], coeff [B, A, K], det [B, n]")
    _on(det, proto.device, "det")
    _on(counts, proto.device, "counts")
    if not det.is_contiguous() or not counts.is_contiguous():
        raise ValueError("assemble_masks_indexed: det and counts must be contiguous")
    B, K, H, W = proto.shape
    A = coeff.shape[1]
    n = det.shape[1]
    if coeff.shape != (B, A, K) or det.shape != (B, n) or det.dtype != torch.int64 or counts.shape != (B,) \
            or counts.dtype != torch.int32:
        raise ValueError("assemble_masks_indexed: need coeff [B, A, K], det [B, n] int64, counts [B] int32")
    bptr = None
    if box is not None:
        box = _on(_f32(box, "box"), proto.device, "box")
        if box.shape != (B, A, 4):
            raise ValueError(f"assemble_masks_indexed: box {tuple(box.shape)} must be [{B}, {A}, 4]")
        bptr = ctypes.c_void_p(box.data_ptr())
    out = _lib.check_out(out, (B, n, H, W), proto.device, "assemble_masks_indexed")
    _lib.check(_lib.lib().tv_yolact_assemble_masks_indexed(
        ctypes.c_void_p(proto.data_ptr()), _lib.strides(proto, 4), B, K, H, W, ctypes.c_void_p(coeff.data_ptr()), bptr,
        A, ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(counts.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
        _lib.stream_of(proto.device)), "assemble_masks_indexed")
    return out


REC = 8  # floats per detection record: anchor, class id, its probability, foreground confidence, y, x, h, w


def detection_records(classification: torch.Tensor, box: torch.Tensor, det: torch.Tensor, counts: torch.Tensor,
                      out: Optional[torch.Tensor] = None, confidence_out: Optional[torch.Tensor] = None):
    """The node's per-detection outputs (yolact_node.py:129, 139-141) for B images in one launch:
    classification [B, A, C+1] logits, box [B, A, 4], det [B, n] int64 / counts [B] int32 (BatchedNMS
    outputs) -> (records [B, n, 8] fp32, confidence). A record is the anchor index, the class id
    (argmax of the logits over all C+1 columns, column 0 the background, the lowest index on a tie),
    that class's softmax probability, the largest foreground probability (what nms ranks by) and the
    box (y, x, h, w) bit for bit. `confidence_out`: a [B, n, C+1] fp32 buffer for the whole softmax
    rows (the node's confidence_np), returned as the second value (None without it). Every row of
    both is written by every call; rows at or past counts[b] are zero. `out`: a caller-owned records
    buffer. No allocation with both buffers given, no host synchronisation."""
    for t, name, dt in ((classification, "classification", torch.float32), (box, "box", torch.float32),
                        (det, "det", torch.int64), (counts, "counts", torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"detection_records: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dt:
            raise ValueError(f"detection_records: {name} must be {dt}, got {t.dtype}")
    if classification.dim() != 3 or box.dim() != 3 or det.dim() != 2 or counts.dim() != 1:
        raise ValueError("detection_records: need classification [B, A, C+1], box [B, A, 4], det [B, n], counts [B]")
    B, A, C1 = classification.shape
    n = det.shape[1]
    if tuple(box.shape) != (B, A, 4) or det.shape[0] != B or counts.shape[0] != B:
        raise ValueError(f"detection_records: classification {list(classification.shape)}, box {list(box.shape)}, "
                         f"det {list(det.shape)}, counts {list(counts.shape)} do not belong together")
    if C1 < 2 or A < 1 or A > 1 << 24:
        raise ValueError("detection_records: need >= 2 classes (with the background) and 1 <= anchors <= 2^24 "
                         "(the anchor index is stored as fp32)")
    _lib.require_gpu()
    dev = classification.device
    for t, name in ((classification, "classification"), (box, "box"), (det, "det"), (counts, "counts")):
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"detection_records: {name} is on {t.device}; every tensor must be on one CUDA device")
        if not t.is_contiguous():
            raise ValueError(f"detection_records: {name} must be contiguous")
    out = _lib.check_out(out, (B, n, REC), dev, "detection_records")
    cptr = None
    if confidence_out is not None:
        confidence_out = _lib.check_out(confidence_out, (B, n, C1), dev, "detection_records confidence")
        cptr = ctypes.c_void_p(confidence_out.data_ptr())
    _lib.check(_lib.lib().tv_yolact_detection_records(
        ctypes.c_void_p(classification.data_ptr()), ctypes.c_void_p(box.data_ptr()), ctypes.c_void_p(det.data_ptr()),
        ctypes.c_void_p(counts.data_ptr()), B, A, C1, n, ctypes.c_void_p(out.data_ptr()), cptr,
        _lib.stream_of(dev)), "detection_records")
    return out, confidence_out


# ---- the instance masks at frame size (csrc/yolact_frame.hip; the contract is tv_yolact_frame_masks') ----

# matplotlib's tab10 as the reference's callers turn it into a colour (evaluate_batch.py:109-111,
# utils/plot.py:121-123): row i is int(255 * (v / 255)) of the i-th tab10 entry v
TAB10 = torch.tensor([[31, 119, 180], [255, 127, 14], [44, 160, 44], [214, 39, 40], [148, 103, 189], [140, 86, 75],
                      [227, 119, 194], [127, 127, 127], [188, 189, 34], [23, 190, 207]], dtype=torch.uint8)
FRAME_MODES = {"bilinear": 0, "nearest": 1}  # TV_FRAME_*


class FrameMasks(NamedTuple):
    """bits [B, n, H, ceil(W / 32)] uint32 (pixel x is bit x % 32 of word x // 32; zero at x >= W and in
    rows at or past counts[b]), area [B, n] int32 (set bits per row), overlay [B, H, W, 3] uint8 or None
    without frames."""
    bits: torch.Tensor
    area: torch.Tensor
    overlay: Optional[torch.Tensor]


def _frame_mode(mode):
    if mode not in FRAME_MODES:
        raise ValueError(f"frame_masks: mode must be one of {sorted(FRAME_MODES)}, got {mode!r}")
    return FRAME_MODES[mode]


def _frame_out(t, shape, dtype, device, name):
    """A caller-owned output of frame_masks (or a fresh one): contiguous, of exactly `shape`."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device \
            or not t.is_contiguous():
        raise ValueError(f"frame_masks: out.{name} must be a contiguous {dtype} {list(shape)} tensor on {device}")
    return t


def frame_masks(masks: torch.Tensor, counts: torch.Tensor, size, mode: str = "bilinear",
                det: Optional[torch.Tensor] = None, box: Optional[torch.Tensor] = None,
                frames: Optional[torch.Tensor] = None, records: Optional[torch.Tensor] = None,
                palette: Optional[torch.Tensor] = None, out: Optional[FrameMasks] = None) -> FrameMasks:
    """The instance masks at frame size for B images in one step: masks [B, n, mh, mw] fp32
    (assemble_masks_indexed output) and counts [B] int32 -> F.interpolate(mask, size, mode) > 0.5
    (evaluate_batch.py:98-102 with "bilinear", yolact_node.py:135,143,184 with "nearest") as packed bits
    and their areas; the up-sampled fp32 mask is never stored. size = (H, W) of the frame.

    det [B, n] int64 with box [B, A, 4] (BatchedNMS / box_decode outputs; both or neither): for masks
    that were assembled with `box`, which are zero outside it, only the box crop is evaluated — the
    same bits, fewer pixels read. frames [B, H, W, 3] uint8 with records [B, n, 8] (detection_records)
    also blends every mask into the frame as utils/plot.py:148-152 does, detection by detection:
    overlay = uint8(0.5 colour + 0.5 pixel), colour = palette[min(class id, len(palette) - 1)]; palette
    [n_colours, 3] uint8 (None: TAB10). Rectangles and text are the caller's to draw from the records.
    `out`: caller-owned FrameMasks buffers (overlay may be None without frames); with them and a device
    palette a call allocates nothing and never synchronises. Every element is written by every call."""
    code = _frame_mode(mode)
    for t, name, dt in ((masks, "masks", torch.float32), (counts, "counts", torch.int32)) + \
            (((det, "det", torch.int64), (box, "box", torch.float32)) if det is not None or box is not None else ()) + \
            (((frames, "frames", torch.uint8), (records, "records", torch.float32)) if frames is not None else ()) + \
            (((palette, "palette", torch.uint8),) if palette is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"frame_masks: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dt:
            raise ValueError(f"frame_masks: {name} must be {dt}, got {t.dtype}")
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"frame_masks: size must be (H, W) with H, W >= 1, got {size}")
    H, W = int(size[0]), int(size[1])
    if masks.dim() != 4 or counts.dim() != 1 or counts.shape[0] != masks.shape[0]:
        raise ValueError(f"frame_masks: need masks [B, n, mh, mw] and counts [B], got {list(masks.shape)}, "
                         f"{list(counts.shape)}")
    B, n, mh, mw = masks.shape
    if mh < 1 or mw < 1:
        raise ValueError(f"frame_masks: masks must be [B, n, mh, mw] with mh, mw >= 1, got {list(masks.shape)}")
    if det is not None and (tuple(det.shape) != (B, n) or box.dim() != 3 or box.shape[0] != B or box.shape[1] < 1
                            or box.shape[2] != 4):
        raise ValueError(f"frame_masks: need det [{B}, {n}] and box [{B}, A, 4], got {list(det.shape)}, "
                         f"{list(box.shape)}")
    if frames is not None and (tuple(frames.shape) != (B, H, W, 3) or tuple(records.shape) != (B, n, REC)):
        raise ValueError(f"frame_masks: need frames [{B}, {H}, {W}, 3] and records [{B}, {n}, {REC}], got "
                         f"{list(frames.shape)}, {list(records.shape)}")
    if palette is not None and (palette.dim() != 2 or palette.shape[0] < 1 or palette.shape[1] != 3):
        raise ValueError(f"frame_masks: palette must be [n_colours >= 1, 3], got {list(palette.shape)}")
    _lib.require_gpu()
    dev = masks.device
    if frames is not None and palette is None:
        palette = TAB10.to(dev)
    for t, name in ((masks, "masks"), (counts, "counts"), (det, "det"), (box, "box"), (frames, "frames"),
                    (records, "records"), (palette if frames is not None else None, "palette")):
        if t is None:
            continue
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"frame_masks: {name} is on {t.device}; every tensor must be on one CUDA device")
        if not t.is_contiguous():
            raise ValueError(f"frame_masks: {name} must be contiguous")
    ob, oa, oo = (None, None, None) if out is None else out
    bits = _frame_out(ob, (B, n, H, (W + 31) // 32), torch.uint32, dev, "bits")
    area = _frame_out(oa, (B, n), torch.int32, dev, "area")
    overlay = None if frames is None else _frame_out(oo, (B, H, W, 3), torch.uint8, dev, "overlay")
    if B * n == 0:  # nothing is launched: the overlay is the frame
        if overlay is not None:
            overlay.copy_(frames)
        return FrameMasks(bits, area, overlay)

    def vp(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().tv_yolact_frame_masks(
        vp(masks), mh, mw, vp(counts), B, n, H, W, code, 0 if det is None else 1, vp(det), vp(box),
        0 if box is None else box.shape[1], vp(frames), vp(records) if frames is not None else None,
        vp(palette) if frames is not None else None, palette.shape[0] if frames is not None else 0, vp(bits), vp(area),
        vp(overlay), _lib.stream_of(dev)), "frame_masks")
    return FrameMasks(bits, area, overlay)


def unpack_frame_masks(bits: torch.Tensor, W: int) -> torch.Tensor:
    """bits [..., H, ceil(W / 32)] (uint32 or int32, host or device) -> bool [..., H, W]: the
    reference's `mask > 0.5` array. Plain torch ops."""
    W = int(W)
    if not isinstance(bits, torch.Tensor) or bits.dtype not in (torch.uint32, torch.int32) or bits.dim() < 2:
        raise ValueError("unpack_frame_masks: bits must be a uint32 / int32 tensor [..., H, ceil(W / 32)]")
    if W < 1 or bits.shape[-1] != (W + 31) // 32:
        raise ValueError(f"unpack_frame_masks: {bits.shape[-1]} words per row do not hold W = {W} pixels")
    words = bits.contiguous().view(torch.int32).unsqueeze(-1)
    shifts = torch.arange(32, dtype=torch.int32, device=bits.device)
    px = ((words >> shifts) & 1).ne(0)  # (an arithmetic shift: the sign fill never reaches bit 0)
    return px.reshape(*bits.shape[:-1], bits.shape[-1] * 32)[..., :W]


def pack_frame_masks(mask: torch.Tensor) -> torch.Tensor:
    """bool [..., H, W] -> bits [..., H, ceil(W / 32)] uint32 in frame_masks' layout (the inverse of
    unpack_frame_masks; plain torch ops, for references and tests)."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() < 2:
        raise ValueError("pack_frame_masks: mask must be a bool tensor [..., H, W]")
    W = mask.shape[-1]
    ww = (W + 31) // 32
    m = torch.zeros(mask.shape[:-1] + (ww * 32,), dtype=torch.int64, device=mask.device)
    m[..., :W] = mask
    weights = torch.ones(32, dtype=torch.int64, device=mask.device) << torch.arange(32, device=mask.device)
    words = (m.reshape(mask.shape[:-1] + (ww, 32)) * weights).sum(-1)  # < 2^32
    return (words - ((words >> 31) << 32)).to(torch.int32).view(torch.uint32)


class DeviceFrameMasks:
    """Static-buffer frame_masks for a fixed (B, K) and frame size, as DeviceLocalizer: a call launches
    on the current stream into the preallocated `bits` [B, K, H, ceil(W / 32)], `area` [B, K] and
    `overlay` [B, H, W, 3] (overlay=False: none is held and no frames are taken), with no allocation
    and no host synchronisation, so it captures in a graph behind the detector's other steps. `palette`:
    [n_colours, 3] uint8 (None: TAB10), copied to the device once."""

    def __init__(self, B, K, frame_hw, device, overlay=True, palette=None):
        if int(B) < 0 or int(K) < 0 or len(frame_hw) != 2 or min(int(v) for v in frame_hw) < 1:
            raise ValueError(f"DeviceFrameMasks needs B, K >= 0 and frame_hw = (H, W), got {B}, {K}, {frame_hw}")
        self.B, self.K = int(B), int(K)
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceFrameMasks needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        H, W = self.frame_hw
        dev = self.device
        self.bits = torch.zeros((self.B, self.K, H, (W + 31) // 32), dtype=torch.uint32, device=dev)
        self.area = torch.zeros((self.B, self.K), dtype=torch.int32, device=dev)
        self.overlay = torch.zeros((self.B, H, W, 3), dtype=torch.uint8, device=dev) if overlay else None
        pal = TAB10 if palette is None else palette
        if not isinstance(pal, torch.Tensor) or pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[0] < 1 \
                or pal.shape[1] != 3:
            raise ValueError("DeviceFrameMasks: palette must be a uint8 [n_colours >= 1, 3] tensor")
        self.palette = pal.to(dev).contiguous()
        self._host = None

    def __call__(self, masks, counts, mode="bilinear", det=None, box=None, frames=None, records=None) -> FrameMasks:
        """frame_masks into the static buffers; frames (with records) only when built with overlay."""
        if frames is not None and self.overlay is None:
            raise ValueError("DeviceFrameMasks was built with overlay=False: it takes no frames")
        if not isinstance(masks, torch.Tensor) or masks.dim() != 4 or tuple(masks.shape[:2]) != (self.B, self.K):
            raise ValueError(f"DeviceFrameMasks built for masks [{self.B}, {self.K}, mh, mw]")
        return frame_masks(masks, counts, self.frame_hw, mode, det, box, frames, records,
                           self.palette if frames is not None else None,
                           FrameMasks(self.bits, self.area, self.overlay if frames is not None else None))

    def host(self, overlay=True) -> FrameMasks:
        """The last call's (bits, area, overlay or None) on the host: copied to pinned memory, one
        synchronisation. Views of this object's pinned mirror, overwritten by the next host()."""
        srcs = [self.bits.view(-1).view(torch.uint8), self.area.view(-1).view(torch.uint8)]
        if overlay and self.overlay is not None:
            srcs.append(self.overlay.view(-1))
        if self._host is None:
            total = self.bits.numel() * 4 + self.area.numel() * 4 + (0 if self.overlay is None else self.overlay.numel())
            self._host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
        parts, off = [], 0
        with torch.cuda.device(self.device):
            for s in srcs:
                parts.append(self._host[off:off + s.numel()])
                parts[-1].copy_(s, non_blocking=True)
                off += s.numel()
            torch.cuda.current_stream(self.device).synchronize()
        return FrameMasks(parts[0].view(torch.uint32).view(self.bits.shape),
                          parts[1].view(torch.int32).view(self.area.shape),
                          parts[2].view(self.overlay.shape) if len(parts) > 2 else None)


# ---- the neck and the head: everything of Yolact.forward after the backbone (model.py:34-60) ----

def yolact_head_state_dict(state_dict):
    """A reference Yolact state_dict without its `_backbone.*` entries: what YolactHead.load_state_dict
    takes (`_feature_pyramid.*`, `_masknet.*`, `_prediction_head.*`)."""
    return {k: v for k, v in state_dict.items() if not k.startswith("_backbone.")}


def _maps(backbone_outputs, in_depths):
    """The backbone maps as contiguous fp32 NCHW tensors of one CUDA device and batch; refuses
    anything else before a launch."""
    maps = tuple(backbone_outputs)
    if len(maps) != len(in_depths):
        raise ValueError(f"expected {len(in_depths)} backbone maps, got {len(maps)}")
    _lib.require_gpu()
    dev, B = maps[0].device, maps[0].shape[0]
    out = []
    for i, (m, c) in enumerate(zip(maps, in_depths)):
        if m.dim() != 4 or m.shape[1] != c or m.shape[0] != B:
            raise ValueError(f"backbone map {i}: expected [{B}, {c}, H, W], got {tuple(m.shape)}")
        if m.device != dev or not m.is_cuda:
            raise ValueError(f"backbone map {i} is on {m.device}; every map must be on one CUDA device "
                             f"(map 0 is on {dev})")
        out.append(m.to(torch.float32).contiguous())
    return out


def _outputs(out, shapes, device, what):
    """Caller-owned output buffers (or fresh ones): contiguous fp32 of exactly `shapes` on `device`."""
    if out is None:
        return [torch.empty(s, dtype=torch.float32, device=device) for s in shapes]
    out = list(out)
    if len(out) != len(shapes):
        raise ValueError(f"{what}: out must hold {len(shapes)} tensors, got {len(out)}")
    return [_lib.check_out(o, s, device, f"{what} out[{i}]") for i, (o, s) in enumerate(zip(out, shapes))]


class FeaturePyramid(NativeModule):
    """feature_pyramid.py:8-58: the backbone maps (c3, c4, c5) -> the tuple of len(in_depths) +
    n_fpn_downsample_layers maps [B, F, h, w]. Parameters keep the reference keys
    (`_lateral_layers.i.*`, `_downsample_layers.i.*`, `_prediction_layers.i.*`). One native call:
    lateral 1x1 convs, the top-down bilinear up-sampling + add in place (any per-axis ratio, as
    F.interpolate(mode="bilinear")), 3x3 convs + LeakyReLU. Each result is a [B, F, h, w] view of an
    fp32 NHWC tensor; `out`: caller-owned NHWC buffers [B, h, w, F]."""

    def __init__(self, in_depths, config, precision: str = "fp32"):
        super().__init__()
        self.in_depths = tuple(int(c) for c in in_depths)
        self.config = config
        self._init_native(precision)
        layout = param_layout(_head_desc(self.in_depths, [(1, 1)] * len(self.in_depths), config, "fp32", True))
        populate(self, layout, seed_layout=layout)

    def engine(self, device, sizes):
        return self._engine(device, (tuple(sizes),),
                            lambda: _head_desc(self.in_depths, sizes, self.config, self.precision, True), self.state_dict)

    def forward_nhwc(self, backbone_outputs, out=None):
        maps = _maps(backbone_outputs, self.in_depths)
        dev = maps[0].device
        eng = self.engine(dev, tuple((m.shape[2], m.shape[3]) for m in maps))
        B = maps[0].shape[0]
        outs = _outputs(out, [(B, h, w, cp) for h, w, _, cp in model_io(eng.desc)[1]], dev, "FeaturePyramid")
        eng.forward_multi(maps, outs)
        return tuple(outs)

    def forward(self, backbone_outputs, out=None):
        return tuple(o.permute(0, 3, 1, 2) for o in self.forward_nhwc(backbone_outputs, out))


class PredictionHead(NativeModule):
    """prediction_head.py:9-143: the parameters of the one head shared by every FPN level, in the
    reference layout (the Bottleneck blocks as torchvision's: conv1, bn1, conv2, bn2, conv3, bn3,
    bias-free convs). It runs inside YolactHead's native plan, once per level with the same weights;
    on its own it has no forward."""

    def __init__(self, config, precision: str = "fp32"):
        super().__init__()
        self.config = config
        self._init_native(precision)
        F = int(config.feature_depth)
        layout = [(k[len("_prediction_head."):], s) for k, s in param_layout(_head_desc((F,), [(1, 1)], config, "fp32"))
                  if k.startswith("_prediction_head.")]
        populate(self, layout, seed_layout=layout)

    def forward(self, fpn_output):
        raise RuntimeError("PredictionHead runs inside YolactHead's native plan (one launch sequence for the "
                           "neck, every level's head and the protonet); call YolactHead((c3, c4, c5))")


class YolactHead(NativeModule):
    """Everything of Yolact.forward after the backbone (model.py:34-60): (c3, c4, c5) ->
    (classification [B, A, C+1], box_encoding [B, A, 4], mask_coeff [B, A, k], anchor [1, A, 4],
    mask_prototype [B, k, 4h, 4w]), all fp32, in one native call. The three anchor-indexed tensors are
    contiguous; mask_prototype is a view of an fp32 NHWC tensor (Masknet's layout).

    Sub-modules `_feature_pyramid`, `_masknet`, `_prediction_head` are the reference Yolact's
    attributes, so `load_state_dict(yolact_head_state_dict(reference_yolact.state_dict()))` works.
    Two reference quirks are kept: one PredictionHead for every level, and rows ordered pixel-major
    with the aspect ratio innermost ((y * W + x) * n_ar + a, prediction_head.py:112-113) while
    get_anchor lays its anchors out one block per aspect ratio.

    `out`: caller-owned (classification, box_encoding, mask_coeff, mask_prototype NHWC [B, 4h, 4w, k
    rounded up to 4]) buffers — with them a step allocates nothing and can be captured in a graph
    after one eager call on the capture stream.

    Only this module's `precision` counts for its forward (`set_precision` changes it); the
    sub-modules hold the parameters."""

    def __init__(self, in_depths, config, precision: str = "fp32"):
        super().__init__()
        self.in_depths = tuple(int(c) for c in in_depths)
        self.config = config
        self._init_native(precision)
        self._feature_pyramid = FeaturePyramid(self.in_depths, config, precision)
        self._masknet = Masknet(config, precision)
        self._prediction_head = PredictionHead(config, precision)
        self._anchors = {}

    def set_precision(self, precision: str):
        """The head's one precision. The sub-modules are used here as parameter holders: their own
        `precision` and engine caches serve only a direct call of `_feature_pyramid(...)` or
        `_masknet(...)`, never this module's forward; they are kept equal to the head's."""
        for m in self.modules():
            if isinstance(m, NativeModule):
                NativeModule.set_precision(m, precision)
        return self

    def head_state_dict(self):
        return yolact_head_state_dict(self.state_dict())

    def anchor(self, level_sizes, device):
        """torch.cat of get_anchor over the FPN levels (model.py:47-58), [1, A, 4], cached."""
        key = (tuple(level_sizes), device)
        a = self._anchors.get(key)
        if a is None:
            a = torch.cat([get_anchor(i, s, self.config) for i, s in enumerate(level_sizes)], dim=1)
            self._anchors = {key: a.to(device, torch.float32).contiguous()}
            a = self._anchors[key]
        return a

    def level_sizes(self, sizes):
        """(h, w) of every FPN level for backbone maps of `sizes`."""
        out = [tuple(int(v) for v in s) for s in sizes]
        for _ in range(int(self.config.n_fpn_downsample_layers)):
            out.append(((out[-1][0] - 1) // 2 + 1, (out[-1][1] - 1) // 2 + 1))
        return out

    def engine(self, device, sizes):
        return self._engine(device, (tuple(sizes),),
                            lambda: _head_desc(self.in_depths, sizes, self.config, self.precision), self.head_state_dict)

    def forward(self, backbone_outputs, out=None):
        maps = _maps(backbone_outputs, self.in_depths)
        sizes = tuple((m.shape[2], m.shape[3]) for m in maps)
        levels = self.level_sizes(sizes)
        if len(levels) > len(self.config.anchor_scales):
            raise ValueError(f"{len(levels)} FPN levels but {len(self.config.anchor_scales)} anchor_scales")
        dev = maps[0].device
        eng = self.engine(dev, sizes)
        B = maps[0].shape[0]
        (A, _, c1, _), _, (_, _, k, _), (ph, pw, _, kp) = model_io(eng.desc)[1]
        outs = _outputs(out, [(B, A, c1), (B, A, 4), (B, A, k), (B, ph, pw, kp)], dev, "YolactHead")
        eng.forward_multi(maps, outs)
        return outs[0], outs[1], outs[2], self.anchor(levels, dev), outs[3][..., :k].permute(0, 3, 1, 2)


def _image(img):
    """The network input as a contiguous fp32 NCHW tensor on its CUDA device; refuses anything else
    before a launch."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"expected img [batch, 3, in_h, in_w], got {tuple(img.shape)}")
    _lib.require_gpu()
    if not img.is_cuda:
        raise ValueError(f"img is on {img.device}; it must be on a CUDA device")
    return img.to(torch.float32).contiguous()


def _check_normalisation(config):
    """The kernels normalise with the ImageNet constants: refuse a config that asks for others."""
    if config is None:
        return
    mean = tuple(float(v) for v in getattr(config, "img_mean", IMAGENET_MEAN))
    std = tuple(float(v) for v in getattr(config, "img_stddev", IMAGENET_STDDEV))
    if mean != IMAGENET_MEAN or std != IMAGENET_STDDEV:
        raise ValueError(f"img_mean {mean} / img_stddev {std}: the frame kernels normalise with the ImageNet values "
                         f"{IMAGENET_MEAN} / {IMAGENET_STDDEV} only; normalise yourself and call forward(img)")


def _frames(frames, size, config):
    """Camera frames as uint8 [B, H, W, 3] and the model's (in_h, in_w) (`size`, or the frames' own):
    Centernet.forward_frames' argument checks, every one of them before the GPU is needed."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"frames must be a torch tensor, got {type(frames).__name__}")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [B, H, W, 3], got {frames.dtype} {list(frames.shape)}")
    if frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError(f"frames must be uint8 [B, H, W, 3] with H, W >= 1, got {list(frames.shape)}")
    if size is None:
        in_h, in_w = frames.shape[1], frames.shape[2]
    else:
        if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError(f"size must be (in_h, in_w), got {size}")
        in_h, in_w = int(size[0]), int(size[1])
    _check_normalisation(config)
    return frames, (in_h, in_w)


def _frames_on_gpu(frames):
    """The frames, contiguous, on their CUDA device (the current one for host frames)."""
    _lib.require_gpu()
    return (frames if frames.is_cuda else frames.cuda()).contiguous()


class Resnet101Backbone(NativeModule):
    """yolact/model/backbone.py:9-32 (the reference's class name; the network is torchvision's
    resnet18): img [B, 3, H, W] -> (c3, c4, c5), the outputs of layer2.1.bn2, layer3.1.bn2 and
    layer4.1.bn2 — each the last block's second BatchNorm, before the residual add and the ReLU —
    with 128 / 256 / 512 channels at strides 8 / 16 / 32. One native call (TV_ARCH_RESNET18): the
    7x7 stem, the 3x3 max-pool, the BasicBlocks as GEMMs with BatchNorm folded and the residual as a
    K-segment. Each result is a [B, C, h, w] view of an fp32 NHWC tensor; `out`: caller-owned NHWC
    buffers [B, h, w, C].

    The parameters sit in the sub-module `_feature_extractor` under torchvision's names (`conv1`,
    `bn1`, `layerL.B.conv1|bn1|conv2|bn2`, `layerL.0.downsample.0|1`; no `fc`), so the `_backbone.*`
    part of a reference Yolact state_dict loads unchanged. torchvision is not a dependency: the
    names and the forward are restated from its resnet.py."""

    depths = (128, 256, 512)

    def __init__(self, config=None, precision: str = "fp32"):
        super().__init__()
        self.config = config
        self._init_native(precision)
        layout = [("_feature_extractor." + k, s) for k, s in param_layout(resnet18_desc())]
        populate(self, layout, seed_layout=layout)

    @staticmethod
    def map_sizes(in_h, in_w):
        """(h, w) of c3, c4, c5 for an in_h x in_w image: (x - 1) // 2 + 1 per stride-2 stage."""
        def half(v):
            return (int(v) - 1) // 2 + 1
        h, w = half(half(in_h)), half(half(in_w))
        out = []
        for _ in range(3):
            h, w = half(h), half(w)
            out.append((h, w))
        return out

    def backbone_state_dict(self):
        n = len("_feature_extractor.")
        return {k[n:]: v for k, v in self.state_dict().items()}

    def engine(self, device, in_h, in_w):
        return self._engine(device, (in_h, in_w), lambda: resnet18_desc(in_h, in_w, self.precision),
                            self.backbone_state_dict)

    def _run(self, x, H, W, out, u8):
        B, dev = x.shape[0], x.device
        eng = self.engine(dev, H, W)
        outs = _outputs(out, [(B, h, w, cp) for h, w, _, cp in model_io(eng.desc)[1]], dev, "Resnet101Backbone")
        if u8:
            eng.forward_multi_u8(x, outs)
        else:
            eng.forward_multi([x], outs)
        return tuple(outs)

    def forward_nhwc(self, img, out=None):
        x = _image(img)
        return self._run(x, x.shape[2], x.shape[3], out, False)

    def forward(self, img, out=None):
        return tuple(o.permute(0, 3, 1, 2) for o in self.forward_nhwc(img, out))

    def forward_frames(self, frames, size=None, out=None):
        """Raw uint8 RGB camera frames [B, H, W, 3] (or [H, W, 3]) through the node's preprocessing
        (yolact_node.py:109-111: ToTensor -> Resize(size) -> Normalize) and forward: exactly what
        forward returns. size = (in_h, in_w) of the model (None: the frames' own size). At the model
        size the frames go straight to the native plan (ToTensor + Normalize in the stem kernel's LUT;
        in fp32 in the staging kernel); otherwise `preprocess` resizes + normalises into the fp32
        forward() input first."""
        from .centernet import preprocess
        frames, (in_h, in_w) = _frames(frames, size, self.config)
        frames = _frames_on_gpu(frames)
        if (in_h, in_w) != (frames.shape[1], frames.shape[2]):
            return self.forward(preprocess(frames, in_h, in_w), out)
        return tuple(o.permute(0, 3, 1, 2) for o in self._run(frames, in_h, in_w, out, True))


class Yolact(YolactHead):
    """model.py:18-60. With `backbone=Resnet101Backbone(config, precision)` the whole forward from the
    image is one native plan (TV_ARCH_YOLACT): the backbone's taps feed the lateral convs straight
    from the arena, one engine per (device, image size, precision), and a reference
    `Yolact.state_dict()` loads as a whole with strict=True. With any other backbone module
    `backbone(img)` -> the three maps runs first (e.g. a torchvision feature extractor under
    PyTorch-ROCm; `in_depths` defaults to its `depths` attribute, else the reference backbone's
    (128, 256, 512)), then YolactHead. Returns YolactHead's five tensors; `out` as YolactHead's."""

    def __init__(self, config, backbone: Optional[nn.Module] = None, precision: str = "fp32", in_depths=None):
        if in_depths is None:
            in_depths = getattr(backbone, "depths", (128, 256, 512))
        super().__init__(in_depths, config, precision)
        if backbone is not None:
            self._backbone = backbone
        if self._native():
            if self.in_depths != Resnet101Backbone.depths:
                raise ValueError(f"in_depths {self.in_depths}: the native backbone gives {Resnet101Backbone.depths}")
            self.set_precision(precision)

    def _native(self):
        return isinstance(getattr(self, "_backbone", None), Resnet101Backbone)

    def forward(self, img, out=None):
        if getattr(self, "_backbone", None) is None:
            raise RuntimeError("Yolact was built without a backbone: the ResNet is not part of this library. Pass "
                               "backbone=<nn.Module returning (c3, c4, c5)>, or run your backbone yourself and call "
                               "YolactHead((c3, c4, c5))")
        if not self._native():
            return super().forward(self._backbone(img), out)
        x = _image(img)
        return self._run(x, x.shape[2], x.shape[3], out, False)

    def _image_engine(self, dev, H, W):
        """The one-plan engine of an H x W image on `dev` and its FPN level sizes."""
        levels = self.level_sizes(Resnet101Backbone.map_sizes(H, W))
        if len(levels) > len(self.config.anchor_scales):
            raise ValueError(f"{len(levels)} FPN levels but {len(self.config.anchor_scales)} anchor_scales")
        c = self.config
        eng = self._engine(dev, ("img", H, W),
                           lambda: yolact_desc(H, W, int(c.feature_depth), int(c.n_fpn_downsample_layers),
                                               int(c.n_classes), int(c.n_prototype_masks),
                                               len(c.anchor_aspect_ratios), _head_layers(c), self.precision),
                           self.state_dict)
        return eng, levels

    def output_shapes(self, B, H, W, device):
        """The shapes of the four `out` buffers (classification, box_encoding, mask_coeff, mask_prototype
        NHWC) of a B-frame forward of H x W images on the native backbone."""
        eng, _ = self._image_engine(device, H, W)
        (A, _, c1, _), _, (_, _, k, _), (ph, pw, _, kp) = model_io(eng.desc)[1]
        return [(B, A, c1), (B, A, 4), (B, A, k), (B, ph, pw, kp)]

    def _run(self, x, H, W, out, u8):
        B, dev = x.shape[0], x.device
        eng, levels = self._image_engine(dev, H, W)
        k = model_io(eng.desc)[1][2][2]
        outs = _outputs(out, self.output_shapes(B, H, W, dev), dev, "Yolact")
        if u8:
            eng.forward_multi_u8(x, outs)
        else:
            eng.forward_multi([x], outs)
        return outs[0], outs[1], outs[2], self.anchor(levels, dev), outs[3][..., :k].permute(0, 3, 1, 2)

    def forward_frames(self, frames, size=None, out=None):
        """Raw uint8 RGB camera frames [B, H, W, 3] (or [H, W, 3]) through the node's preprocessing
        (yolact_node.py:109-111: ToTensor -> Resize(size) -> Normalize) and forward (:119): exactly what
        forward returns. size = (in_h, in_w) of the model (None: the frames' own size). With the native
        backbone and frames at the model size, ToTensor + Normalize run inside the plan's first kernel
        and the fp32 image never exists; otherwise `preprocess` resizes + normalises into the fp32
        forward() input first."""
        from .centernet import preprocess
        frames, (in_h, in_w) = _frames(frames, size, self.config)
        if getattr(self, "_backbone", None) is None:
            return self.forward(None)  # (raises: no backbone)
        frames = _frames_on_gpu(frames)
        if not self._native() or (in_h, in_w) != (frames.shape[1], frames.shape[2]):
            return self.forward(preprocess(frames, in_h, in_w), out)
        return self._run(frames, in_h, in_w, out, True)

    def invalidate(self):
        super().invalidate()
        self._detectors = {}

    def detect(self, frames, top_k, iou_threshold, confidence_threshold, depth=None, camera=None, frame_masks=None):
        """The node's callback from the camera frame to the detections (yolact_node.py:109-143) in one
        call: uint8 RGB frames [B, H, W, 3] (or [H, W, 3]) of any size, resized to (config.in_h,
        config.in_w), through a cached YolactDetector (native backbone). depth (uint16 millimetres,
        [dh, dw] or [B, dh, dw], numpy or torch) with camera = (fx, fy, cx, cy) also localises every
        detection (:177-193). Returns YolactDetections(records [B, K, 8] and counts [B] on the host,
        the masks [B, K, 4h, 4w] on the device — the detector's static buffer, overwritten by the next
        call —, points [B, K, 8] on the host or None); K = min(top_k, anchors). One device-to-host
        synchronisation. frame_masks = "bilinear" or "nearest" also gives the masks at the frames' own
        size (YolactDetector's frame_masks step): bits, area and overlay, on the device like `masks`
        (the detector's static buffers; `unpack_frame_masks(bits, W)` is the reference's bool array)."""
        from .localize import _host_depth
        frames, _ = _frames(frames, None, self.config)
        if int(top_k) < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        if (depth is None) != (camera is None):
            raise ValueError("depth and camera = (fx, fy, cx, cy) go together")
        if camera is not None and len(camera) != 4:
            raise ValueError(f"camera must be (fx, fy, cx, cy), got {camera}")
        if not self._native():
            raise ValueError("detect needs the native backbone: Yolact(config, backbone=Resnet101Backbone(config))")
        if frame_masks is not None:
            _frame_mode(frame_masks)
        B = frames.shape[0]
        if depth is not None:
            depth = _host_depth(depth, max(B, 1))
        frames = _frames_on_gpu(frames)
        dev = frames.device
        hw, size = (frames.shape[1], frames.shape[2]), (int(self.config.in_h), int(self.config.in_w))
        key = (dev.index, B, hw, size, int(top_k), self.precision, self._version_key(), frame_masks)
        det = getattr(self, "_detectors", {}).get(key)
        if det is None:
            det = YolactDetector(self, B, hw, int(top_k), dev, size, frame_masks=frame_masks)
            self._detectors = {key: det}
        res = det(frames, iou_threshold, confidence_threshold, None if depth is None else depth.to(dev), camera)
        records, counts, points = det.host()
        return YolactDetections(records.clone(), counts.clone(), res.masks, None if points is None else points.clone(),
                                res.bits, res.area, res.overlay)


class YolactDetections(NamedTuple):
    """records [B, K, 8] fp32 (anchor, class id, its probability, foreground confidence, y, x, h, w;
    rows at or past counts[b] zero), counts [B] int32, masks [B, K, 4h, 4w] fp32 on the device (rows
    past counts[b] are not written), points [B, K, 8] fp32 (DeviceLocalizer's x, y, z, valid, n_pixels,
    depth_sum, e_x, e_y) or None without depth. With the detector's frame_masks step: bits [B, K, H,
    ceil(W / 32)] uint32, area [B, K] int32 and overlay [B, H, W, 3] uint8 (None for the fp32 entry) of
    FrameMasks at the frame size, on the device; None without it."""
    records: torch.Tensor
    counts: torch.Tensor
    masks: torch.Tensor
    points: Optional[torch.Tensor]
    bits: Optional[torch.Tensor] = None
    area: Optional[torch.Tensor] = None
    overlay: Optional[torch.Tensor] = None


class YolactDetector:
    """The node's callback from the camera frames to the detections (yolact_node.py:109-143) for one
    (B, frame size) with static device buffers: forward_frames(out=...) -> box_decode -> BatchedNMS ->
    assemble_masks_indexed -> detection_records and, with depth, DeviceLocalizer.masks(bound_by_box).
    `model`: a Yolact on the native backbone; frame_hw = (H, W) of the camera frames; size = (in_h,
    in_w) of the model (None: the frames' own size; another size runs `preprocess` into a static fp32
    image first); K = min(top_k, anchors). frame_masks = "bilinear" or "nearest" adds the masks at
    frame_hw after detection_records (DeviceFrameMasks `frame`, bounded by the boxes): bits and area,
    and the overlay onto the uint8 frames of the call (the fp32 entry has no frames: overlay None).
    With None (the default) the step does not exist: no launch, no buffer.

    A call launches on the current stream, allocates nothing and never synchronises, so it can be
    captured in a graph after one eager call on the capture stream (the pattern of YolactHead(out=...)).
    The buffers — `head_out` (classification, box_encoding, mask_coeff, mask_prototype NHWC), `box`
    [B, A, 4], `det` [B, K] int64, `masks` [B, K, 4h, 4w], `points` [B, K, 8], and `records` [B, K, 8] +
    `counts` [B] as views of one allocation `packed` (DeviceDecoder's layout: one copy carries both) —
    are overwritten by every call. Mask rows past counts[b] are not written (they start as zeros)."""

    def __init__(self, model, B, frame_hw, top_k, device, size=None, frame_masks=None):
        from .localize import DeviceLocalizer
        if frame_masks is not None:
            _frame_mode(frame_masks)
        if not isinstance(model, Yolact) or not model._native():
            raise ValueError("YolactDetector needs a Yolact on the native backbone "
                             "(Yolact(config, backbone=Resnet101Backbone(config)))")
        if int(B) < 1 or int(top_k) < 1 or len(frame_hw) != 2 or min(int(v) for v in frame_hw) < 1:
            raise ValueError(f"YolactDetector needs B >= 1, top_k >= 1 and frame_hw = (H, W), got {B}, {top_k}, {frame_hw}")
        _check_normalisation(model.config)
        self.model, self.B, self.top_k = model, int(B), int(top_k)
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.size = self.frame_hw if size is None else (int(size[0]), int(size[1]))
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"YolactDetector needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        shapes = model.output_shapes(self.B, self.size[0], self.size[1], dev)
        self.head_out = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        (_, A, _), _, _, (_, ph, pw, _) = shapes
        self.img = None if self.size == self.frame_hw else \
            torch.empty((self.B, 3) + self.size, dtype=torch.float32, device=dev)
        self.box = torch.empty((self.B, A, 4), dtype=torch.float32, device=dev)
        self.nms = BatchedNMS(self.B, A, self.top_k, dev)
        self.K = K = self.nms.K
        nrec = self.B * K * REC
        self.packed = torch.zeros((nrec + self.B) * 4, dtype=torch.uint8, device=dev)
        self.records = self.packed[:nrec * 4].view(torch.float32).view(self.B, K, REC)
        self.counts = self.nms.counts = self.packed[nrec * 4:].view(torch.int32)  # (the NMS writes them here)
        self.det = self.nms.det
        self.masks = torch.zeros((self.B, K, ph, pw), dtype=torch.float32, device=dev)
        self.localizer = DeviceLocalizer(self.B, K, dev)
        self.points = self.localizer.out
        self.frame_mode = frame_masks
        self.frame = None if frame_masks is None else DeviceFrameMasks(self.B, K, self.frame_hw, dev)
        self._overlaid = False
        self._localized = False
        self._host = None

    def __call__(self, frames, iou_threshold, confidence_threshold, depth=None, camera=None):
        """frames: uint8 [B, H, W, 3] of the detector's frame size on its device — or the normalised
        fp32 image [B, 3, in_h, in_w] (the fp32 entry, for frames preprocessed elsewhere). depth: uint16
        millimetres [1 or B, dh, dw] on the device, with camera = (fx, fy, cx, cy). Returns
        YolactDetections of the static device buffers (points None without depth)."""
        from .centernet import preprocess
        m = self.model
        if (depth is None) != (camera is None):
            raise ValueError("depth and camera = (fx, fy, cx, cy) go together")
        if camera is not None and len(camera) != 4:
            raise ValueError(f"camera must be (fx, fy, cx, cy), got {camera}")
        if not isinstance(frames, torch.Tensor) or frames.device != self.device:
            raise ValueError(f"frames must be a tensor on {self.device}")
        if frames.dtype == torch.float32:
            if tuple(frames.shape) != (self.B, 3) + self.size:
                raise ValueError(f"the fp32 image must be {[self.B, 3, *self.size]}, got {list(frames.shape)}")
            pred = m.forward(frames, out=self.head_out)
            u8 = None
        else:
            frames, _ = _frames(frames, None, m.config)
            if tuple(frames.shape) != (self.B,) + self.frame_hw + (3,):
                raise ValueError(f"YolactDetector built for frames {[self.B, *self.frame_hw, 3]}, got {list(frames.shape)}")
            if self.img is None:
                pred = m.forward_frames(frames, out=self.head_out)
            else:
                pred = m.forward(preprocess(frames, self.size[0], self.size[1], out=self.img), out=self.head_out)
            u8 = frames
        classification, box_encoding, mask_coeff, anchor, mask_prototype = pred
        box = box_decode(box_encoding, anchor, m.config, out=self.box)
        det, counts = self.nms(classification, box, iou_threshold, confidence_threshold)
        assemble_masks_indexed(mask_prototype, mask_coeff, box, det, counts, out=self.masks)
        detection_records(classification, box, det, counts, out=self.records)
        self._localized = depth is not None
        if self._localized:
            fx, fy, cx, cy = camera
            self.localizer.masks(self.masks, counts, det, box, depth, fx, fy, cx, cy, bound_by_box=True)
        points = self.points if self._localized else None
        if self.frame is None:
            return YolactDetections(self.records, self.counts, self.masks, points)
        self._overlaid = u8 is not None
        fm = self.frame(self.masks, counts, self.frame_mode, det, box, u8, None if u8 is None else self.records)
        return YolactDetections(self.records, self.counts, self.masks, points, fm.bits, fm.area, fm.overlay)

    def host_frame_masks(self) -> FrameMasks:
        """FrameMasks(bits, area, overlay or None) of the last call on the host: copied to pinned memory
        with one synchronisation; views of the pinned mirror, overwritten by the next call of this."""
        if self.frame is None:
            raise ValueError("this YolactDetector was built without frame_masks")
        return self.frame.host(overlay=self._overlaid)

    def host(self):
        """(records [B, K, 8], counts [B], points [B, K, 8] or None) of the last call on the host: the
        packed records (and the points) copied to pinned memory, one synchronisation. The tensors are
        views of the detector's pinned mirror, overwritten by the next host()."""
        nrec = self.B * self.K * REC * 4
        if self._host is None:
            self._host = torch.empty(self.packed.numel() + nrec, dtype=torch.uint8, pin_memory=True)
        h = self._host
        with torch.cuda.device(self.device):
            h[:self.packed.numel()].copy_(self.packed, non_blocking=True)
            if self._localized:
                h[self.packed.numel():].copy_(self.points.view(-1).view(torch.uint8), non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        rec = h[:nrec].view(torch.float32).view(self.B, self.K, REC)
        cnt = h[nrec:self.packed.numel()].view(torch.int32)
        pts = h[self.packed.numel():].view(torch.float32).view(self.B, self.K, REC) if self._localized else None
        return rec, cnt, pts
