"""Drop-in `Centernet` / `Prediction` / `get_head_channels` (reference
src/tauv_vision/centernet/model/centernet.py:13-142) backed by the native MI355X engine.

The module keeps the reference state_dict layout exactly (keys, shapes, order), so
`load_state_dict(torch.load(path))` of a reference checkpoint works unchanged; the
forward pass is one native call (all convolutions as fused MFMA implicit GEMMs, see
csrc/planner.cpp) and returns the reference's `Prediction`, whose tensors are channel
slices of one fp32 NHWC head tensor (same shapes and values, different strides).
"""
import ctypes
import threading
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib
from .config import ObjectConfigSet
from .dla import DLABackbone, populate
from .engine import NativeEngine
from .native import NativeModule
from .weights import model_desc, dla34_desc, param_layout

_GRAPH_LOCK = threading.RLock()  # the forward graph cache's launches and captures (all models)


@dataclass
class Prediction:
    heatmap: torch.Tensor                      # [B, n_labels, out_h, out_w]
    keypoint_heatmap: Optional[torch.Tensor]   # [B, n_keypoints, out_h, out_w]
    keypoint_affinity: Optional[torch.Tensor]  # [B, n_keypoints, 2, out_h, out_w]
    size: torch.Tensor                         # [B, out_h, out_w, 2]
    offset: torch.Tensor                       # [B, out_h, out_w, 2]
    roll_bin: Optional[torch.Tensor]           # [B, out_h, out_w, 4]
    roll_offset: Optional[torch.Tensor]
    pitch_bin: Optional[torch.Tensor]
    pitch_offset: Optional[torch.Tensor]
    yaw_bin: Optional[torch.Tensor]
    yaw_offset: Optional[torch.Tensor]
    depth: Optional[torch.Tensor]              # [B, out_h, out_w, 1]


def get_head_channels(object_config: ObjectConfigSet) -> List[int]:
    """centernet.py:114-142: heatmap, [keypoint heatmap, keypoint affinity], size, offset,
    [yaw bin/offset], [pitch bin/offset], [roll bin/offset], [depth]."""
    out = [object_config.n_labels]
    if object_config.train_keypoints:
        out += [object_config.n_keypoints, 2 * object_config.n_keypoints]
    out += [2, 2]
    for flag in (object_config.train_yaw, object_config.train_pitch, object_config.train_roll):
        if flag:
            out += [4, 4]
    if object_config.train_depth:
        out.append(1)
    return out


def prediction_fields(object_config: ObjectConfigSet):
    """Field -> (first channel, channel count), following the reference's pop order
    (centernet.py:77-90): after size/offset it assigns roll, pitch, yaw — although
    get_head_channels created the angle heads yaw, pitch, roll — then depth."""
    widths = get_head_channels(object_config)
    starts = [sum(widths[:i]) for i in range(len(widths))]
    order = ["heatmap"]
    if object_config.train_keypoints:
        order += ["keypoint_heatmap", "keypoint_affinity"]
    order += ["size", "offset"]
    for axis, flag in (("roll", object_config.train_roll), ("pitch", object_config.train_pitch),
                       ("yaw", object_config.train_yaw)):
        if flag:
            order += [f"{axis}_bin", f"{axis}_offset"]
    if object_config.train_depth:
        order.append("depth")
    return {name: (starts[i], widths[i]) for i, name in enumerate(order)}


def prediction_from_nhwc(out: torch.Tensor, object_config: ObjectConfigSet) -> Prediction:
    fields = {f: None for f in Prediction.__dataclass_fields__}
    for name, (s, n) in prediction_fields(object_config).items():
        t = out[..., s:s + n]
        if name in ("heatmap", "keypoint_heatmap"):
            t = t.permute(0, 3, 1, 2)
        elif name == "keypoint_affinity":
            B, H, W, _ = t.shape
            t = t.unflatten(3, (n // 2, 2)).permute(0, 3, 4, 1, 2)
        fields[name] = t
    return Prediction(**fields)


class _NativeModel(NativeModule):
    """The reference forward API shared by Centernet and CenterpointDLA34, behind a cache of captured
    forward graphs. Subclasses provide `_desc(in_h, in_w)` (the native model description)."""

    def _init_native(self, object_config, precision):
        super()._init_native(precision)
        self.object_config = object_config
        self.head_channels = get_head_channels(object_config)
        # hipGraph replay behind forward()/forward_frames(): a (kind, shape) seen before is replayed
        # from a captured graph instead of launched op by op (set False for eager launches only)
        self.graph_replay = True
        self._graphs = {}

    def invalidate(self):
        super().invalidate()
        self._graphs = {}
        self._detectors = {}

    def _device_for(self, t: torch.Tensor) -> torch.device:
        """`t`'s GPU; a host tensor goes to the parameters' GPU (the current one if they are on the host)."""
        return _lib.current_cuda(t if t.is_cuda else next(self.parameters()))

    def engine(self, device: torch.device, in_h: int, in_w: int) -> NativeEngine:
        return self._engine(device, (in_h, in_w), lambda: self._desc(in_h, in_w), self.state_dict)

    # -- graph cache ------------------------------------------------------------------
    def _launch(self, eng: NativeEngine, kind: str, x: torch.Tensor) -> torch.Tensor:
        """One engine forward of `x` (kind "f32": normalised NCHW, "u8": NHWC frames) on the caller's
        stream, returning a fresh fp32 NHWC head tensor. Per (caller stream, kind, shape): the first
        call runs eagerly; the second captures the forward once as a hipGraph on a private stream
        (static input / output buffers, the engine workspace keyed to that stream: an eager warm-up
        there, then the capture); every later call copies the input in, replays the graph on the
        caller's stream and returns a copy of the output — so results never alias a later call's,
        as the reference's fresh tensors. Eager when graph_replay is off, while the caller's stream
        is capturing, or if the capture failed (graph_failures). Threads (rospy runs one callback
        thread per camera, centernet_node.py:58-65): launches are enqueued under one lock, so a
        capture never sees another thread's launches; the GPU work of different streams still
        overlaps."""
        fwd = eng.forward_u8 if kind == "u8" else eng.forward
        if x.shape[0] == 0:  # an empty batch: the reference's convolutions return empty outputs
            return eng.alloc_out(0)
        if not self.graph_replay or torch.cuda.is_current_stream_capturing():
            return fwd(x)
        cur = torch.cuda.current_stream(eng.device)
        key = (id(eng), eng.generation, cur.cuda_stream, kind, tuple(x.shape))
        with _GRAPH_LOCK:
            ent = self._graphs.get(key)
            if ent is None:  # first sight: eager (the node's warm-up forward, centernet_node.py:50)
                self._graphs = {k: v for k, v in self._graphs.items() if k[0] == id(eng) and k[1] == eng.generation}
                self._graphs[key] = {"graph": None, "failed": False}
                return fwd(x)
            if ent["failed"]:
                return fwd(x)
            if ent["graph"] is None:
                try:
                    side = torch.cuda.Stream(eng.device)
                    inp = torch.empty_like(x, memory_format=torch.contiguous_format)
                    out = eng.alloc_out(x.shape[0])
                    side.wait_stream(cur)
                    with torch.cuda.stream(side):
                        inp.copy_(x)
                        fwd(inp, out)  # workspace for (side, B) made outside the capture
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                            fwd(inp, out)
                    cur.wait_stream(side)
                    ent.update(graph=graph, stream=side, inp=inp, out=out)
                except RuntimeError as e:  # keep the model usable: this (kind, shape) stays eager
                    import warnings
                    warnings.warn(f"tauv_vision_amd: hipGraph capture failed ({e}); eager launches for {key[3:]}")
                    ent["failed"] = True
                    self.graph_failures = getattr(self, "graph_failures", 0) + 1
                    return fwd(x)
            ent["inp"].copy_(x)
            ent["graph"].replay()
            return ent["out"].clone()

    # -- reference API --------------------------------------------------------------
    def forward(self, img: torch.Tensor) -> Prediction:
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"expected img [batch, 3, in_h, in_w], got {tuple(img.shape)}")
        dev = self._device_for(img)
        img = img.to(dev, torch.float32).contiguous()
        eng = self.engine(dev, img.shape[2], img.shape[3])
        return prediction_from_nhwc(self._launch(eng, "f32", img), self.object_config)

    def forward_frames(self, frames: torch.Tensor, size=None) -> Prediction:
        """Raw uint8 RGB camera frames [B, H, W, 3] (or [H, W, 3]) through the node's
        preprocessing (centernet_node.py:90-92): ToTensor -> Resize(size) -> Normalize(ImageNet).
        size = (in_h, in_w) of the model (None: the frames' own size). At the model size the
        resize is the identity and ToTensor + Normalize are fused into the stem kernel; otherwise
        one kernel resizes + normalises (tv_preprocess_u8) into the fp32 forward() input."""
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [B, H, W, 3]")
        dev = self._device_for(frames)
        frames = frames.to(dev).contiguous()
        in_h, in_w = (frames.shape[1], frames.shape[2]) if size is None else (int(size[0]), int(size[1]))
        eng = self.engine(dev, in_h, in_w)
        if (in_h, in_w) == (frames.shape[1], frames.shape[2]):
            return prediction_from_nhwc(self._launch(eng, "u8", frames), self.object_config)
        return prediction_from_nhwc(self._launch(eng, "f32", preprocess(frames, in_h, in_w)), self.object_config)

    def detect(self, frames: torch.Tensor, model_config, n_detections: int = 100, score_threshold: float = 0.3,
               angles: bool = False):
        """detect(frames) == decode(forward(preprocess(frames)), ...): camera frames of any size,
        resized to (model_config.in_h, model_config.in_w) like the node. angles=True: decode_oriented
        with the model's own object config, so Detection.roll / .pitch / .yaw are filled for the labels
        that train them."""
        from .decode import decode, decode_oriented
        pred = self.forward_frames(frames, (model_config.in_h, model_config.in_w))
        if angles:
            return decode_oriented(pred, model_config, self.object_config, n_detections, score_threshold)
        return decode(pred, model_config, n_detections, score_threshold)

    def detect_keypoints(self, frames, model_config, n_detections: int = 10, keypoint_n_detections: int = 50,
                         score_threshold: float = 0.6, keypoint_score_threshold: float = 0.3, depth=None, camera=None,
                         M_projection=None, poses: bool = False, min_points: int = 6):
        """The CenterNet node's callback from the camera frames to the matched keypoints and the 3-D
        points (centernet_node.py:90-178) in one call: uint8 RGB frames [B, H, W, 3] (or [H, W, 3]) of
        any size, resized to (model_config.in_h, model_config.in_w), through a cached CenternetDetector.
        depth (uint16 millimetres, [dh, dw] or [B, dh, dw], numpy or torch) with camera = (fx, fy, cx,
        cy), or with M_projection (the node's matrix: fx, fy, cx, cy = M[0,0], M[1,1], M[0,2], M[1,2]),
        also localises every object. Returns CenternetDetections of host tensors (points None without
        depth). One device-to-host synchronisation. The defaults are the node's (:116-117, :124).
        poses=True: camera (or M_projection) also gives every object with at least min_points matched
        keypoints its pose (the node's commented-out solvePnP use, :183-191), with or without depth;
        returns CenternetPoseDetections (the same fields, then `poses` [B, K, 16])."""
        from .localize import _host_depth
        from .yolact import _frames, _frames_on_gpu
        frames, _ = _frames(frames, None, None)
        if camera is None and M_projection is not None and (depth is not None or poses):
            import numpy as np
            M = np.asarray(M_projection, dtype=np.float64)
            if M.ndim != 2 or M.shape[0] < 2 or M.shape[1] < 3:
                raise ValueError(f"M_projection must be at least 2 x 3, got {list(M.shape)}")
            camera = (float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2]))
        if (depth is None) != (camera is None) and not (poses and depth is None):
            raise ValueError("depth goes with camera = (fx, fy, cx, cy) or M_projection")
        if camera is not None and len(camera) != 4:
            raise ValueError(f"camera must be (fx, fy, cx, cy), got {camera}")
        B = frames.shape[0]
        if depth is not None:
            depth = _host_depth(depth, max(B, 1))
        frames = _frames_on_gpu(frames)
        dev = frames.device
        hw = (frames.shape[1], frames.shape[2])
        key = (dev.index, B, hw, int(model_config.in_h), int(model_config.in_w), int(n_detections),
               int(keypoint_n_detections), self.precision, self._version_key()) + ((True,) if poses else ())
        det = getattr(self, "_detectors", {}).get(key)
        if det is None:
            det = CenternetDetector(self, B, hw, model_config, n_detections, keypoint_n_detections, dev, poses=poses)
            self._detectors = {key: det}
        with torch.cuda.device(dev):
            if poses:
                det(frames, score_threshold, keypoint_score_threshold, None if depth is None else depth.to(dev), camera,
                    min_points)
                return CenternetPoseDetections(*[None if t is None else t.clone() for t in det.host()])
            det(frames, score_threshold, keypoint_score_threshold, None if depth is None else depth.to(dev), camera)
            return CenternetDetections(*[None if t is None else t.clone() for t in det.host()])


class CenternetDetections(NamedTuple):
    """KeypointRecords' arrays (decode.py: `records` [B, K, 10] / `counts` [B] of the objects,
    `keypoint_records` [B, K_kp, 10] / `keypoint_counts` [B], `slot_kp` [B, K, max_slots], `n_matched`
    [B, K], `kp_det` [B, K_kp]) plus `points` [B, K, 8] fp32 (DeviceLocalizer's x, y, z, valid, n_pixels,
    depth_sum, e_x, e_y per object) or None without depth."""
    records: torch.Tensor
    counts: torch.Tensor
    keypoint_records: torch.Tensor
    keypoint_counts: torch.Tensor
    slot_kp: torch.Tensor
    n_matched: torch.Tensor
    kp_det: torch.Tensor
    points: Optional[torch.Tensor]


class CenternetPoseDetections(NamedTuple):
    """CenternetDetections' fields, then `poses` [B, K, 16] fp32 (tv_solve_poses: R row-major, t, valid, n
    points, rms reprojection error in pixels, LM iterations per object) or None without a camera."""
    records: torch.Tensor
    counts: torch.Tensor
    keypoint_records: torch.Tensor
    keypoint_counts: torch.Tensor
    slot_kp: torch.Tensor
    n_matched: torch.Tensor
    kp_det: torch.Tensor
    points: Optional[torch.Tensor]
    poses: Optional[torch.Tensor]


class CenternetDetector:
    """The CenterNet node's callback (centernet_node.py:90-178) for one (B, frame size) with static device
    buffers: the engine's forward into `head_out` (from the uint8 frames; frames of another size than
    (model_config.in_h, in_w) go through `preprocess` into the static fp32 `img` first) ->
    DeviceKeypointDecoder (object decode, keypoint decode, matching) -> with depth,
    DeviceLocalizer.boxes on the object records with the node's 0.4 / 10 / 1. `model`: a
    CenterpointDLA34 or a Centernet whose object config trains keypoints.

    A call launches on the current stream, allocates nothing and never synchronises, and it calls the
    engine itself (not the module's graph cache): the whole step can be captured in one graph after one
    eager call on the capture stream. `decoder`'s buffers and `points` [B, K, 8] are overwritten by every
    call.

    poses=True: the decoder carries a `poses` section in its packed buffer and, whenever a camera is given
    (with or without depth), tv_solve_poses runs after the matching; calls and host() return
    CenternetPoseDetections. Still one packed copy, nothing allocated per call, capturable."""

    def __init__(self, model, B, frame_hw, model_config, n_detections=10, keypoint_n_detections=50, device=None,
                 poses=False):
        from .decode import DeviceKeypointDecoder
        from .localize import DeviceLocalizer
        if not isinstance(model, _NativeModel):
            raise ValueError("CenternetDetector needs a CenterpointDLA34 or a Centernet")
        oc = model.object_config
        if not oc.train_keypoints or oc.n_keypoints < 1:
            raise ValueError("CenternetDetector needs a model with keypoint heads (object_config.train_keypoints)")
        if int(B) < 1 or len(frame_hw) != 2 or min(int(v) for v in frame_hw) < 1:
            raise ValueError(f"CenternetDetector needs B >= 1 and frame_hw = (H, W), got {B}, {frame_hw}")
        _lib.require_gpu()
        dev = next(model.parameters()).device if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"CenternetDetector needs a GPU device, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.model, self.model_config, self.B, self.device = model, model_config, int(B), dev
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.size = (int(model_config.in_h), int(model_config.in_w))
        self.engine = model.engine(dev, *self.size)
        self.head_out = self.engine.alloc_out(self.B)
        self.prediction = prediction_from_nhwc(self.head_out, oc)
        self.img = None if self.size == self.frame_hw else \
            torch.empty((self.B, 3) + self.size, dtype=torch.float32, device=dev)
        _, C, H, W = self.prediction.heatmap.shape
        self.K = int(n_detections)
        self.with_poses = bool(poses)
        self.decoder = DeviceKeypointDecoder(self.B, C, oc.n_keypoints, H, W, self.K, int(keypoint_n_detections), oc,
                                             dev, poses=self.with_poses)
        self._posed = False
        self.localizer = DeviceLocalizer(self.B, self.K, dev)
        self.points = self.localizer.out
        self._localized = False
        self._host = None

    def __call__(self, frames, score_threshold, keypoint_score_threshold, depth=None, camera=None, min_points=6):
        """frames: uint8 [B, H, W, 3] of the detector's frame size on its device — or the normalised fp32
        image [B, 3, in_h, in_w] (the fp32 entry, for frames preprocessed elsewhere). depth: uint16
        millimetres [1 or B, dh, dw] on the device, with camera = (fx, fy, cx, cy). Returns
        CenternetDetections of the static device buffers (points None without depth). A detector built
        with poses=True also takes camera without depth and returns CenternetPoseDetections (poses None
        without a camera); min_points: the fewest matched keypoints a pose is solved from (6..32)."""
        if (depth is None) != (camera is None) and not (self.with_poses and depth is None):
            raise ValueError("depth and camera = (fx, fy, cx, cy) go together")
        if camera is not None and len(camera) != 4:
            raise ValueError(f"camera must be (fx, fy, cx, cy), got {camera}")
        if self.with_poses and camera is not None:
            import math
            if not 6 <= int(min_points) <= 32:
                raise ValueError(f"min_points must be in 6..32, got {min_points}")
            if not all(math.isfinite(float(v)) for v in camera[:2]) or float(camera[0]) == 0 or float(camera[1]) == 0:
                raise ValueError("fx and fy must be finite and not 0")
        if not isinstance(frames, torch.Tensor) or frames.device != self.device:
            raise ValueError(f"frames must be a tensor on {self.device}")
        dec = self.decoder
        if depth is not None:
            from .localize import check_boxes_args
            check_boxes_args(self.B, self.K, dec.records, dec.counts, depth, camera[0], camera[1], self.device)
        if frames.dtype == torch.float32:
            if tuple(frames.shape) != (self.B, 3) + self.size or not frames.is_contiguous():
                raise ValueError(f"the fp32 image must be contiguous {[self.B, 3, *self.size]}, got {list(frames.shape)}")
            self.engine.forward(frames, self.head_out)
        else:
            if frames.dtype != torch.uint8 or tuple(frames.shape) != (self.B,) + self.frame_hw + (3,) \
                    or not frames.is_contiguous():
                raise ValueError(f"CenternetDetector built for contiguous uint8 frames {[self.B, *self.frame_hw, 3]}, "
                                 f"got {frames.dtype} {list(frames.shape)}")
            if self.img is None:
                self.engine.forward_u8(frames, self.head_out)
            else:
                self.engine.forward(preprocess(frames, self.size[0], self.size[1], out=self.img), self.head_out)
        res = dec(self.prediction, self.model_config, score_threshold, keypoint_score_threshold)
        self._localized = depth is not None
        if self._localized:
            fx, fy, cx, cy = camera
            self.localizer.boxes(res.records, res.counts, depth, fx, fy, cx, cy, 0.4, 10.0, 1.0)
        if not self.with_poses:
            return CenternetDetections(*res, self.points if self._localized else None)
        self._posed = camera is not None
        if self._posed:
            dec.solve(self.model_config, camera, min_points)
        return CenternetPoseDetections(*res, self.points if self._localized else None,
                                       dec.poses if self._posed else None)

    def host(self):
        """CenternetDetections of the last call on the host: the decoder's packed buffer (and the points)
        copied to pinned memory, one synchronisation. The tensors are views of the detector's pinned
        mirror, overwritten by the next host()."""
        dec = self.decoder
        n = dec.packed.numel()
        if self._host is None:
            self._host = torch.empty(n + self.points.numel() * 4, dtype=torch.uint8, pin_memory=True)
        h = self._host
        with torch.cuda.device(self.device):
            h[:n].copy_(dec.packed, non_blocking=True)
            if self._localized:
                h[n:].copy_(self.points.view(-1).view(torch.uint8), non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        pts = h[n:].view(torch.float32).view(tuple(self.points.shape)) if self._localized else None
        if not self.with_poses:
            return CenternetDetections(*dec._views(h[:n]), pts)
        o = dec._offsets[-1]
        poses = h[o:n].view(torch.float32).view(tuple(dec.poses.shape)) if self._posed else None
        return CenternetPoseDetections(*dec._views(h[:n]), pts, poses)


class Centernet(_NativeModel):
    """centernet.py:32-92. `precision`: "fp32" (exact-f32 MFMA, parity mode), "fp16" or
    "bf16" (fp32 accumulation; throughput mode)."""

    def __init__(self, backbone: DLABackbone, object_config: ObjectConfigSet, precision: str = "fp32"):
        super().__init__()
        self.backbone = backbone
        self._init_native(object_config, precision)
        desc = model_desc(backbone.heights, backbone.channels, backbone.downsamples, self.head_channels)
        layout = [(k, s) for k, s in param_layout(desc) if k.startswith("heads.")]
        self.heads = nn.Module()
        populate(self.heads, [(k[len("heads."):], s) for k, s in layout], seed_layout=layout, prefix="heads.")

    def _desc(self, in_h, in_w):
        return model_desc(self.backbone.heights, self.backbone.channels, self.backbone.downsamples,
                          self.head_channels, in_h, in_w, self.precision)


class CenterpointDLA34(_NativeModel):
    """centerpoint_dla.py:544-578: DLASeg('dla34', heads {'0'..'n-1'}, down_ratio 4,
    final_kernel 1, last_level 5, head_conv 256) under `self.model`, so reference checkpoints
    (keys `model.base...`, `model.dla_up...`, `model.ida_up...`, `model.<i>.{0,2}...`) load
    unchanged. The reference constructor downloads ImageNet DLA-34 weights (get_pose_net,
    :534-541); here the parameters start from the seeded recipe and a checkpoint is loaded
    with load_state_dict. DCNv2 runs natively (csrc/dla34.hip + MFMA GEMM over its columns)."""

    def __init__(self, object_config: ObjectConfigSet, precision: str = "fp32"):
        super().__init__()
        self._init_native(object_config, precision)
        layout = param_layout(dla34_desc(self.head_channels))
        self.model = nn.Module()
        populate(self.model, [(k[len("model."):], s) for k, s in layout], seed_layout=layout, prefix="model.")

    def _desc(self, in_h, in_w):
        return dla34_desc(self.head_channels, in_h, in_w, self.precision)


def preprocess(frames: torch.Tensor, in_h: int, in_w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The node's T.ToTensor -> T.Resize((in_h, in_w)) -> T.Normalize(ImageNet)
    (centernet_node.py:90-92, yolact_node.py:109-111) on the GPU: u8 RGB frames [B, H, W, 3] (or
    [H, W, 3]) at camera resolution -> normalised fp32 [B, 3, in_h, in_w] (bilinear,
    align_corners=False, no antialias: torchvision 0.15.2's tensor Resize). `out`: a caller-owned
    contiguous fp32 [B, 3, in_h, in_w] buffer on the frames' device (no allocation per call)."""
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [B, H, W, 3]")
    _lib.require_gpu()
    frames = (frames if frames.is_cuda else frames.cuda()).contiguous()
    B, H, W, _ = frames.shape
    out = _lib.check_out(out, (B, 3, int(in_h), int(in_w)), frames.device, "preprocess")
    if B == 0:
        return out
    _lib.check(_lib.lib().tv_preprocess_u8(ctypes.c_void_p(frames.data_ptr()), B, H, W, int(in_h), int(in_w),
                                           ctypes.c_void_p(out.data_ptr()), _lib.stream_of(frames.device)),
               "preprocess")
    return out


def initialize_weights(module: nn.Module, excluded_modules=()):
    """centernet.py:103-111 analogue: re-draw every conv/conv-transpose weight xavier-uniform
    and zero its bias (parameter tree leaves with a 4-D weight)."""
    excluded = set()
    for m in excluded_modules:
        excluded.update(id(x) for x in m.modules())
    for sub in module.modules():
        w = sub._parameters.get("weight") if hasattr(sub, "_parameters") else None
        if w is not None and w.dim() == 4 and id(sub) not in excluded:
            with torch.no_grad():
                nn.init.xavier_uniform_(w)
                b = sub._parameters.get("bias")
                if b is not None:
                    b.zero_()
    for m in module.modules():
        if isinstance(m, NativeModule):
            m.invalidate()
