"""Depth localisation of detections on the GPU: the per-detection loops of the two reference
nodes that turn a detection into a camera-frame point from the raw mono16 depth image
(csrc/localize.hip; the contract is in include/tauv_vision_amd.h).

  * box mode (centernet_node.py:139-178): the filled rectangle of +-0.4 w, +-0.4 h around the
    centre, np.sum / np.mean of the positive depth in it, the `< 10` and `z < 1` skips and the
    back-projection through M_projection;
  * mask mode (yolact_node.py:135,143,177-193): F.interpolate (nearest) of every assembled mask
    to the raw image size, np.nanmean(np.where(mask > 0.5, depth, nan)) and the back-projection
    through the camera intrinsics.

`depth` is the uint16 millimetre image itself ([B, dh, dw], or [1, dh, dw] for all images); no
float image and no up-sampled mask is ever stored. Output rows are [x, y, z, valid, n_pixels,
depth_sum, e_x, e_y] fp32.

Differences from the reference:
  * the node hard-codes 640 x 360 (its depth size); here the depth tensor's own size is used;
  * depth is summed exactly in integer millimetres and divided once, where the node sums float64
    metres: depth_sum and z agree to about 1e-14 relative before the fp32 store;
  * a non-finite box gives an invalid row (the node's int() would raise).
"""
import ctypes
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib

OUT = 8  # x, y, z, valid, n_pixels, depth_sum, e_x, e_y


def _require(t, name, dtype, device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU, got a tensor on {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the localizer on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _check_depth(depth, B, device=None):
    _require(depth, "depth", torch.uint16, device)
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"depth must be [B, dh, dw] or [1, dh, dw], got {list(depth.shape)}")
    if depth.shape[0] not in (1, B):
        raise ValueError(f"depth batch {depth.shape[0]} is neither 1 nor B = {B}")
    return depth


def _check_counts(counts, B, device=None):
    _require(counts, "counts", torch.int32, device)
    if tuple(counts.shape) != (B,):
        raise ValueError(f"counts must be [{B}], got {list(counts.shape)}")
    return counts


def _check_camera(fx, fy):
    if float(fx) == 0.0 or float(fy) == 0.0:
        raise ValueError("fx and fy must not be 0")


def check_boxes_args(B, K, records, counts, depth, fx, fy, device=None):
    """The argument checks of DeviceLocalizer.boxes (ValueError before any launch)."""
    _require(records, "records", torch.float32, device)
    if records.dim() != 3 or tuple(records.shape[:2]) != (B, K) or records.shape[2] < 6:
        raise ValueError(f"records must be [{B}, {K}, >= 6] (y, x, h, w in columns 2-5), got {list(records.shape)}")
    _check_counts(counts, B, device)
    _check_depth(depth, B, device)
    _check_camera(fx, fy)


def check_masks_args(B, K, masks, counts, det, box, depth, fx, fy, device=None):
    """The argument checks of DeviceLocalizer.masks (ValueError before any launch)."""
    _require(masks, "masks", torch.float32, device)
    if masks.dim() != 4 or tuple(masks.shape[:2]) != (B, K) or masks.shape[2] < 1 or masks.shape[3] < 1:
        raise ValueError(f"masks must be [{B}, {K}, mh, mw], got {list(masks.shape)}")
    _check_counts(counts, B, device)
    _require(det, "det", torch.int64, device)
    if tuple(det.shape) != (B, K):
        raise ValueError(f"det must be [{B}, {K}], got {list(det.shape)}")
    _require(box, "box", torch.float32, device)
    if box.dim() != 3 or box.shape[0] != B or box.shape[1] < 1 or box.shape[2] != 4:
        raise ValueError(f"box must be [{B}, A, 4], got {list(box.shape)}")
    _check_depth(depth, B, device)
    _check_camera(fx, fy)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class DeviceLocalizer:
    """Static-buffer localisation for a fixed (B, K): `.boxes` / `.masks` launch one kernel on the
    current stream into the preallocated `out` [B, K, 8] fp32 and return it, with no allocation and
    no host synchronisation — forward -> DeviceDecoder -> DeviceLocalizer captures in one HIP graph.
    Every row of `out` is written by every call (rows past counts[b] are zero)."""

    def __init__(self, B, K, device):
        if B < 0 or K < 0:
            raise ValueError(f"B and K must not be negative, got {B}, {K}")
        self.B, self.K = int(B), int(K)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceLocalizer needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.out = torch.zeros((self.B, self.K, OUT), dtype=torch.float32, device=self.device)

    def boxes(self, records, counts, depth, fx, fy, cx, cy, box_scale=0.4, min_depth_sum=10.0, min_z=1.0):
        """centernet_node.py:139-178 for records [B, K, >= 6] (DeviceDecoder.records: y, x, h, w in
        columns 2-5) and counts [B] int32."""
        check_boxes_args(self.B, self.K, records, counts, depth, fx, fy, self.device)
        _lib.check(_lib.lib().tv_localize_boxes(
            _vp(records), records.shape[2], _vp(counts), self.B, self.K, _vp(depth), depth.shape[0], depth.shape[1],
            depth.shape[2], float(box_scale), float(fx), float(fy), float(cx), float(cy), float(min_depth_sum),
            float(min_z), _vp(self.out), _lib.stream_of(self.device)), "localize_boxes")
        return self.out

    def masks(self, masks, counts, det, box, depth, fx, fy, cx, cy, bound_by_box=False, min_depth_sum=0.0,
              min_z=0.0):
        """yolact_node.py:135,143,177-193 for masks [B, K, mh, mw] (assemble_masks_indexed output),
        det [B, K] int64 / counts [B] int32 (BatchedNMS outputs) and box [B, A, 4]. `bound_by_box`:
        scan only the box crop — for masks that were assembled with `box` (zero outside it)."""
        check_masks_args(self.B, self.K, masks, counts, det, box, depth, fx, fy, self.device)
        _lib.check(_lib.lib().tv_localize_masks(
            _vp(masks), masks.shape[2], masks.shape[3], _vp(counts), _vp(det), _vp(box), box.shape[1], self.B, self.K,
            _vp(depth), depth.shape[0], depth.shape[1], depth.shape[2], 1 if bound_by_box else 0, float(fx), float(fy),
            float(cx), float(cy), float(min_depth_sum), float(min_z), _vp(self.out), _lib.stream_of(self.device)),
            "localize_masks")
        return self.out


def _host_depth(depth, B):
    """depth as a uint16 torch tensor [1 or B, dh, dw] (host or device), checked."""
    if isinstance(depth, np.ndarray):
        if depth.dtype != np.uint16:
            raise ValueError(f"depth must be uint16 (mono16 millimetres), got {depth.dtype}")
        depth = torch.from_numpy(np.ascontiguousarray(depth))
    if not isinstance(depth, torch.Tensor):
        raise ValueError(f"depth must be a numpy array or a torch tensor, got {type(depth).__name__}")
    if depth.dtype != torch.uint16:
        raise ValueError(f"depth must be uint16 (mono16 millimetres), got {depth.dtype}")
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"depth must be [H, W] or [B, H, W], got {list(depth.shape)}")
    if depth.shape[0] not in (1, B):
        raise ValueError(f"depth batch {depth.shape[0]} is neither 1 nor the {B} images of the detections")
    return depth.contiguous()


def _device_for(*tensors):
    _lib.require_gpu()
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def localize_detections(detections, depth, M_projection, box_scale=0.4, min_depth_sum=10.0,
                        min_z=1.0) -> List[List[Optional[Tuple[float, float, float]]]]:
    """The CenterNet node's localisation loop (centernet_node.py:139-178) for the output of
    decode() / decode_keypoints() — a list, per image, of Detection / KeypointDetection — or
    `[one image's list]`. depth: uint16 millimetres, numpy or torch, [H, W] (every image) or
    [B, H, W]. Returns per image a list aligned with its detections: (x, y, z) Python floats, or
    None where the node would `continue`. One kernel launch, one device-to-host copy."""
    if not isinstance(detections, (list, tuple)) or any(not isinstance(d, (list, tuple)) for d in detections):
        raise ValueError("detections must be a list of per-image detection lists (pass [dets] for one image)")
    B = len(detections)
    M = np.asarray(M_projection, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] < 2 or M.shape[1] < 3:
        raise ValueError(f"M_projection must be at least 2 x 3, got {list(M.shape)}")
    fx, fy, cx, cy = float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2])
    _check_camera(fx, fy)
    depth = _host_depth(depth, max(B, 1))
    K = max([len(d) for d in detections], default=0)
    if B == 0 or K == 0:
        return [[] for _ in range(B)]
    rec = np.zeros((B, K, 6), dtype=np.float32)
    cnt = np.zeros((B,), dtype=np.int32)
    for b, dets in enumerate(detections):
        cnt[b] = len(dets)
        for k, d in enumerate(dets):
            rec[b, k, 2:6] = (d.y, d.x, d.h, d.w)
    dev = _device_for(depth)
    loc = DeviceLocalizer(B, K, dev)
    out = loc.boxes(torch.from_numpy(rec).to(dev), torch.from_numpy(cnt).to(dev), depth.to(dev), fx, fy, cx, cy,
                    box_scale, min_depth_sum, min_z).cpu().numpy()
    return [[(float(r[0]), float(r[1]), float(r[2])) if r[3] != 0 else None for r in out[b, :cnt[b]]]
            for b in range(B)]


def localize_masks(masks, det, box, depth, fx, fy, cx, cy, counts=None, bound_by_box=False, min_depth_sum=0.0,
                   min_z=0.0) -> np.ndarray:
    """The YOLACT node's localisation loop (yolact_node.py:135,143,177-193). One image: masks
    [n, mh, mw] (assemble_mask output), det [n] int64 (nms output), box [A, 4]; or batched: masks
    [B, n, mh, mw], det [B, n], box [B, A, 4], counts [B] int32 (None = all n). depth: uint16
    millimetres, numpy or torch, [H, W] or [B, H, W]. Returns the host records [n, 8] or [B, n, 8]
    fp32 (x, y, z, valid, n_pixels, depth_sum, e_x, e_y; valid == 0 where the node would `continue`).
    One kernel launch, one device-to-host copy."""
    for t, name, dt in ((masks, "masks", torch.float32), (det, "det", torch.int64), (box, "box", torch.float32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dt:
            raise ValueError(f"{name} must be {dt}, got {t.dtype}")
    single = masks.dim() == 3
    if single:
        if det.dim() != 1 or box.dim() != 2:
            raise ValueError("for masks [n, mh, mw], det must be [n] and box [A, 4]")
        masks, det, box = masks.unsqueeze(0), det.unsqueeze(0), box.unsqueeze(0)
    if masks.dim() != 4 or det.dim() != 2 or box.dim() != 3 or box.shape[-1] != 4:
        raise ValueError("need masks [B, n, mh, mw], det [B, n] and box [B, A, 4]")
    B, n = masks.shape[:2]
    if tuple(det.shape) != (B, n) or box.shape[0] != B:
        raise ValueError(f"batch mismatch: masks {list(masks.shape)}, det {list(det.shape)}, box {list(box.shape)}")
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                               or tuple(counts.shape) != (B,)):
        raise ValueError(f"counts must be an int32 [{B}] tensor")
    _check_camera(fx, fy)
    depth = _host_depth(depth, max(B, 1))
    if B == 0 or n == 0:
        out = np.zeros((B, n, OUT), dtype=np.float32)
        return out[0] if single else out
    dev = _device_for(masks, depth)
    if counts is None:
        counts = torch.full((B,), n, dtype=torch.int32)
    loc = DeviceLocalizer(B, n, dev)
    out = loc.masks(masks.to(dev).contiguous(), counts.to(dev).contiguous(), det.to(dev).contiguous(),
                    box.to(dev).contiguous(), depth.to(dev), fx, fy, cx, cy, bound_by_box, min_depth_sum,
                    min_z).cpu().numpy()
    return out[0] if single else out
