"""Drop-in decode API (reference src/tauv_vision/centernet/model/decode.py:16-324) on the
native gfx950 kernels: sigmoid + 3x3 peak NMS, exact per-image top-K and the per-detection
gather run on the GPU (csrc/decode.hip) and return one packed record buffer, copied to the
host once — instead of one device sync per scalar (decode.py:211-221).

Differences from the reference:
  * Detection.label / .score are 0-d CPU tensors (the reference's are 0-d tensors on the
    prediction's device, decode.py:212-213); y/x/h/w/depth are Python floats.
  * decode()'s y / x: the reference forms (R * i + offset) / in_h in float64 Python arithmetic
    (decode.py:214-215); the kernel evaluates the same expression in double but the record
    stores it as fp32, so y / x are that float64 value rounded to fp32 (relative error
    <= 6e-8). h / w / depth / score are the reference's fp32 values exactly.
  * top-K ties are broken toward the smaller flat index (torch.topk: unspecified).
  * label / y / x use integer division (== the reference's float32 division, decode.py:271-277,
    while C*H*W < 2^24).
  * decode() leaves Detection.roll / pitch / yaw at None, as the reference's does ("TODO: Decode angles",
    decode.py:193-202); decode_oriented() / decode_oriented_records() fill them by the reference's
    angle_decode at the detections' peaks (tv_decode_angles, one launch after the decode).
"""
import ctypes
import threading
from dataclasses import dataclass
from math import atan2, pi
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib

REC = 10  # label, score, y, x, h, w, depth, flat index, aux0, aux1


@dataclass
class Detection:
    label: int
    score: float
    y: float
    x: float
    h: float
    w: float
    yaw: Optional[float] = None
    pitch: Optional[float] = None
    roll: Optional[float] = None
    depth: Optional[float] = None


@dataclass
class KeypointDetection:
    label: int
    score: float
    y: float
    x: float
    w: float
    h: float
    depth: float
    keypoints: List[Optional[Tuple[float, float, float]]]
    keypoint_scores: List[Optional[float]]
    keypoint_affinities: List[Optional[Tuple[float, float, float]]]
    cam_t_object: object


def _gpu(t, name):
    return _lib.require_gpu_tensor(t, name)


def _empty_batch_check(B):
    """The reference's heatmap_detect (decode.py:255-279, and so decode / decode_keypoints) flattens
    the heatmap with reshape(B, -1), which torch refuses for an empty batch: the same error here."""
    if B == 0:
        raise RuntimeError("cannot reshape tensor of 0 elements into shape [0, -1] because the unspecified "
                           "dimension size -1 can be any value and is ambiguous")


def heatmap_nms(heatmap: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """decode.py:239-252: keep values equal to their k x k neighbourhood max, else 0."""
    assert kernel_size >= 1 and kernel_size % 2 == 1
    heatmap = _gpu(heatmap, "heatmap")
    B, C, H, W = heatmap.shape
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=heatmap.device)
    if B == 0:  # the reference's max_pool2d returns the empty batch as is
        return out
    _lib.check(_lib.lib().tv_heatmap_nms(ctypes.c_void_p(heatmap.data_ptr()), _lib.strides(heatmap, 4), B, C, H, W,
                                         kernel_size, 0, ctypes.c_void_p(out.data_ptr()),
                                         _lib.stream_of(heatmap.device)), "heatmap_nms")
    return out


def heatmap_detect(heatmap: torch.Tensor, n_detections: int):
    """decode.py:255-279 -> (index [B,K,2] (y, x), label [B,K], score [B,K])."""
    heatmap = _gpu(heatmap, "heatmap")
    B, C, H, W = heatmap.shape
    n = C * H * W
    _empty_batch_check(B)
    if not 1 <= n_detections <= n:
        raise RuntimeError(f"selected index k out of range (k={n_detections}, n={n})")
    flat = heatmap.reshape(B, n).contiguous()
    dev = heatmap.device
    score = torch.empty((B, n_detections), dtype=torch.float32, device=dev)
    idx32 = torch.empty((B, n_detections), dtype=torch.int32, device=dev)
    index = torch.empty((B, n_detections, 2), dtype=torch.int64, device=dev)
    label = torch.empty((B, n_detections), dtype=torch.int64, device=dev)
    L, s = _lib.lib(), _lib.stream_of(dev)
    _lib.check(L.tv_heatmap_topk(ctypes.c_void_p(flat.data_ptr()), B, n, n_detections,
                                 ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(idx32.data_ptr()), s),
               "heatmap_detect")
    _lib.check(L.tv_index_split(ctypes.c_void_p(idx32.data_ptr()), B, n_detections, H, W,
                                ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(label.data_ptr()), s),
               "heatmap_detect")
    return index, label, score


class DeviceDecoder:
    """Static-buffer decode for a fixed (B, C, H, W, K): launches sigmoid+NMS, exact top-K
    and the record gather on the current stream into preallocated device buffers, with no
    host synchronisation — so a forward + decode step can be captured in a HIP graph.
    `records` is [B, K, 10] fp32, `counts` [B] int32 (see include/tauv_vision_amd.h).
    angles=True appends an `angles` section [B, K, 3] fp32 (roll, pitch, yaw) to `packed`, after the
    counts, for a DeviceAngleDecoder to write (the decode itself never touches it); the prefix layout
    is the same either way."""

    def __init__(self, B, C, H, W, K, device, angles=False):
        if not 1 <= K <= C * H * W:
            raise RuntimeError(f"selected index k out of range (k={K}, n={C * H * W})")
        self.shape = (B, C, H, W, K)
        self.device = torch.device(device)
        need = ctypes.c_int64()
        _lib.check(_lib.lib().tv_decode_workspace_size(B, C, H, W, K, ctypes.byref(need)), "decode")
        self.ws_bytes = need.value
        self.ws = torch.zeros(need.value, dtype=torch.uint8, device=self.device)  # counters zero-filled (tv_decode keeps them so)
        # records and counts (then the angles) in one allocation (`packed`): a single D2H copy carries all
        nrec = B * K * REC
        nang = B * K * 3 if angles else 0
        self.packed = torch.empty((nrec + B + nang) * 4, dtype=torch.uint8, device=self.device)
        self.records = self.packed[:nrec * 4].view(torch.float32).view(B, K, REC)
        self.counts = self.packed[nrec * 4:(nrec + B) * 4].view(torch.int32)
        self.angles = self.packed[(nrec + B) * 4:].view(torch.float32).view(B, K, 3) if angles else None

    def __call__(self, heat, size, offset, depth, mode, ratio, in_h, in_w, thr, aux=None):
        B, C, H, W, K = self.shape
        if tuple(heat.shape) != (B, C, H, W):
            raise ValueError(f"heatmap shape {tuple(heat.shape)} != decoder shape {(B, C, H, W)}")
        dev = self.device

        def ptr_st(t, n, name):
            if t is None:
                return None, None
            t = _gpu(t, name).to(dev)
            return ctypes.c_void_p(t.data_ptr()), _lib.strides(t, n)

        hp, hs = ptr_st(heat, 4, "heatmap")
        sp, ss = ptr_st(size, 4, "size")
        op, os_ = ptr_st(offset, 4, "offset")
        dp, ds = ptr_st(depth, 4, "depth")
        ap, as_ = ptr_st(aux, 5, "keypoint_affinity")
        _lib.check(_lib.lib().tv_decode(hp, hs, sp, ss, op, os_, dp, ds, B, C, H, W, K, mode, ratio, in_h, in_w,
                                        float(thr), ap, as_, ctypes.c_void_p(self.records.data_ptr()),
                                        ctypes.c_void_p(self.counts.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()),
                                        self.ws_bytes, _lib.stream_of(dev)), "decode")
        return self.records, self.counts


ANGLE_AXES = ("roll", "pitch", "yaw")  # Prediction order; the columns of `angles`


def angle_ranges(object_config) -> np.ndarray:
    """float32 [3, n_labels]: the period of roll / pitch / yaw for each label, as the reference's
    angle_range takes it from ObjectConfig.{roll,pitch,yaw}.modulo (loss.py:151-175) — NaN ("not decoded")
    where the label's AngleConfig.train is false or its modulo is None."""
    out = np.full((3, object_config.n_labels), np.nan, dtype=np.float32)
    for a, axis in enumerate(ANGLE_AXES):
        for c, cfg in enumerate(object_config.configs):
            ac = getattr(cfg, axis)
            if ac.train and ac.modulo is not None:
                out[a, c] = ac.modulo
    return out


class DeviceAngleDecoder:
    """Static-buffer roll / pitch / yaw of a DeviceDecoder's records (tv_decode_angles, csrc/decode.hip):
    the reference's angle_decode at the records' peaks, one launch on the current stream with no
    allocation and no host synchronisation, so decode + angles can be captured in one HIP graph. Holds
    the per-label period table `theta_range` [3, n_labels] (angle_ranges) on the device and `angles`
    [B, K, 3] fp32 (roll, pitch, yaw; NaN = not decoded: rows past counts[b], an absent head, a label
    without that angle) — `out`: a caller-owned contiguous buffer for it (a DeviceDecoder's `angles`
    section). Every element is overwritten by every call."""

    def __init__(self, B, K, object_config, device, out=None):
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceAngleDecoder needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if int(B) < 0 or int(K) < 1:
            raise ValueError(f"DeviceAngleDecoder needs B >= 0 and K >= 1, got {B}, {K}")
        self.B, self.K, self.n_labels = int(B), int(K), object_config.n_labels
        self.theta_range = torch.from_numpy(angle_ranges(object_config)).to(self.device)
        self.angles = _lib.check_out(out, (self.B, self.K, 3), self.device, "DeviceAngleDecoder")

    def __call__(self, records, counts, prediction):
        """records [B, K, >= 8] fp32 / counts [B] int32 on the device (DeviceDecoder's), prediction: the
        Prediction they were decoded from. Returns the device `angles`. ValueError before the launch for
        host tensors, other shapes than the decoder's, or a heatmap whose channels are not the labels."""
        B, K = self.B, self.K
        heat = prediction.heatmap
        if not isinstance(heat, torch.Tensor) or heat.dim() != 4 or heat.shape[0] != B or heat.shape[1] != self.n_labels:
            raise ValueError(f"heatmap must be [{B}, {self.n_labels}, H, W], got "
                             f"{list(heat.shape) if isinstance(heat, torch.Tensor) else type(heat)}")
        _, C, H, W = heat.shape
        for name, t, dt in (("records", records, torch.float32), ("counts", counts, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} tensor on {self.device}")
        if records.dim() != 3 or tuple(records.shape[:2]) != (B, K) or tuple(counts.shape) != (B,):
            raise ValueError(f"records / counts shapes {list(records.shape)} / {list(counts.shape)} != decoder's "
                             f"{[B, K, REC]} / {[B]}")
        args = []
        for axis in ANGLE_AXES:
            for part in ("bin", "offset"):
                t = getattr(prediction, f"{axis}_{part}")
                if t is None:
                    args += [None, None]
                    continue
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device \
                        or tuple(t.shape) != (B, H, W, 4):
                    raise ValueError(f"{axis}_{part} must be a float32 {[B, H, W, 4]} tensor on {self.device}")
                args += [ctypes.c_void_p(t.data_ptr()), _lib.strides(t, 4)]
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().tv_decode_angles(vp(records), records.shape[2], vp(counts), *args, vp(self.theta_range),
                                               B, C, H, W, K, vp(self.angles), _lib.stream_of(self.device)),
                   "decode_angles")
        return self.angles


_DECODERS = {}  # (device, B, C, H, W, K, slot, angle table) -> (DeviceDecoder, pinned host mirror, angle decoder)
_DECODERS_LOCK = threading.Lock()
_DECODERS_MAX = 8


def _decoder(dev, B, C, H, W, K, slot=0, object_config=None):
    """The cached decoder of a shape; `slot`: which of several decodes of that shape inside one
    _records_many call (each has its own outputs and host mirror); object_config: with the angle section
    and its DeviceAngleDecoder (keyed by the period table)."""
    table = None if object_config is None else angle_ranges(object_config).tobytes()
    key = (dev.index, B, C, H, W, K, slot, table)
    ent = _DECODERS.get(key)
    if ent is None:
        if len(_DECODERS) >= _DECODERS_MAX:
            _DECODERS.pop(next(iter(_DECODERS)))
        dec = DeviceDecoder(B, C, H, W, K, dev, angles=object_config is not None)
        ang = None if object_config is None else DeviceAngleDecoder(B, K, object_config, dev, out=dec.angles)
        ent = (dec, torch.empty(dec.packed.numel(), dtype=torch.uint8, pin_memory=True), ang)
        _DECODERS[key] = ent
    return ent


def _records_many(calls):
    """Run several device decodes back to back on the current stream, each into a cached decoder
    (static workspace and records: no allocation or zero fill per call), copy every packed record
    buffer to pinned host memory and synchronise ONCE. calls: (heat, size, offset, depth, K, mode,
    ratio, in_h, in_w, thr, aux) tuples, optionally with a 12th element (prediction, object_config):
    tv_decode_angles follows that decode. Two calls of the same (B, C, H, W, K) get a decoder and a host
    buffer each. Returns [(records [B,K,10], counts [B])] host numpy, (records, counts, angles [B,K,3])
    for a call with angles."""
    with _DECODERS_LOCK:
        outs, seen = [], {}
        for call in calls:
            heat, size, offset, depth, K, mode, ratio, in_h, in_w, thr, aux = call[:11]
            oriented = call[11] if len(call) > 11 else None
            heat = _gpu(heat, "heatmap")
            B, C, H, W = heat.shape
            _empty_batch_check(B)
            shape = (heat.device.index, B, C, H, W, K)
            slot = seen[shape] = seen.get(shape, -1) + 1
            dec, host, ang = _decoder(heat.device, B, C, H, W, K, slot, None if oriented is None else oriented[1])
            dec(heat, size, offset, depth, mode, ratio, in_h, in_w, thr, aux)
            if ang is not None:
                ang(dec.records, dec.counts, oriented[0])
            host.copy_(dec.packed, non_blocking=True)
            outs.append((host, B, K, ang is not None))
        torch.cuda.current_stream(heat.device).synchronize()
        res = []
        for host, B, K, has_angles in outs:
            a = host.numpy()
            nrec = B * K * REC
            records = a[:nrec * 4].view(np.float32).reshape(B, K, REC).copy()
            counts = a[nrec * 4:(nrec + B) * 4].view(np.int32).copy()
            if has_angles:
                res.append((records, counts, a[(nrec + B) * 4:].view(np.float32).reshape(B, K, 3).copy()))
            else:
                res.append((records, counts))
        return res


def _records(heat, size, offset, depth, K, mode, ratio, in_h, in_w, thr, aux=None):
    """Run the device decode; returns host numpy records [B,K,10] and counts [B] (one D2H copy)."""
    return _records_many([(heat, size, offset, depth, K, mode, ratio, in_h, in_w, thr, aux)])[0]


def decode_records(prediction, model_config, n_detections: int, score_threshold: float):
    """decode() without the per-detection Python objects: host numpy records [B, K, 10] (label,
    score, y, x, h, w, depth, flat index, -, -; the first counts[b] rows of image b valid) and counts
    [B] int32 — one device decode, one D2H copy, one host synchronisation."""
    return _records(prediction.heatmap, prediction.size, prediction.offset, prediction.depth, n_detections, 0,
                    model_config.downsample_ratio, model_config.in_h, model_config.in_w, score_threshold)


def decode(prediction, model_config, n_detections: int, score_threshold: float) -> List[List[Detection]]:
    """decode.py:179-236."""
    has_depth = prediction.depth is not None
    records, counts = _records(prediction.heatmap, prediction.size, prediction.offset, prediction.depth,
                               n_detections, 0, model_config.downsample_ratio, model_config.in_h, model_config.in_w,
                               score_threshold)
    from .sharding import records_to_detections
    return records_to_detections(records, counts, has_depth)


def decode_oriented_records(prediction, model_config, object_config, n_detections: int, score_threshold: float):
    """decode_records() plus the orientation of every detection: host numpy records [B, K, 10], counts [B]
    and angles [B, K, 3] fp32 (roll, pitch, yaw by the reference's angle_decode with the label's period
    from object_config; NaN where not decoded: rows past counts[b], a prediction without that head, a
    label that does not train that angle or has no modulo). tv_decode and tv_decode_angles launched back
    to back, one D2H copy, one host synchronisation."""
    if object_config.n_labels != prediction.heatmap.shape[1]:
        raise ValueError(f"the object config has {object_config.n_labels} labels, the heatmap "
                         f"{prediction.heatmap.shape[1]} channels")
    return _records_many([(prediction.heatmap, prediction.size, prediction.offset, prediction.depth, n_detections, 0,
                           model_config.downsample_ratio, model_config.in_h, model_config.in_w, score_threshold, None,
                           (prediction, object_config))])[0]


def decode_oriented(prediction, model_config, object_config, n_detections: int,
                    score_threshold: float) -> List[List[Detection]]:
    """decode() with Detection.roll / .pitch / .yaw filled (the reference's "TODO: Decode angles",
    decode.py:193-202, 222-230): Python floats in [0, modulo) where the label trains the angle and the
    prediction has the head, None otherwise. Every other field as decode() gives it."""
    records, counts, angles = decode_oriented_records(prediction, model_config, object_config, n_detections,
                                                      score_threshold)
    from .sharding import records_to_detections
    return records_to_detections(records, counts, prediction.depth is not None, angles)


def decode_keypoints(prediction, model_config, object_config, M_projection, n_detections: int,
                     keypoint_n_detections: int, score_threshold: float, keypoint_score_threshold: float,
                     keypoint_angle_threshold: float, pose: str = "cv2") -> List[List[KeypointDetection]]:
    """decode.py:51-176: objects (no offset / ratio, depth = 1/sigmoid) and keypoints from
    the GPU; the greedy affinity-angle matching (decode.py:100-135) runs on the host over
    at most K x K_kp records. `keypoint_angle_threshold` is unused, as in the reference.
    pose="cv2" (the default): the host _solve_poses, which needs OpenCV once an object has six matched
    keypoints. pose="device": matching and poses on the device (decode_keypoint_poses: tv_match_keypoints,
    tv_solve_poses), cam_t_object = (R float64 [3, 3], t float64 [3, 1]) for the detections whose pose is
    valid; OpenCV is not needed and _solve_poses is not called."""
    if pose not in ("cv2", "device"):
        raise ValueError(f'pose must be "cv2" or "device", got {pose!r}')
    if pose == "device":
        rec, poses = decode_keypoint_poses(prediction, model_config, object_config, M_projection, n_detections,
                                           keypoint_n_detections, score_threshold, keypoint_score_threshold)
        return keypoint_detections_from_records(rec.records, rec.counts, rec.keypoint_records, rec.slot_kp,
                                                prediction.depth is not None, model_config, object_config,
                                                M_projection, poses=poses)
    # both decodes launched back to back, one host synchronisation
    (obj, obj_n), (kp, kp_n) = _records_many([
        (prediction.heatmap, prediction.size, None, prediction.depth, n_detections, 1,
         model_config.downsample_ratio, model_config.in_h, model_config.in_w, score_threshold, None),
        (prediction.keypoint_heatmap, prediction.size, None, None, keypoint_n_detections, 1,
         model_config.downsample_ratio, model_config.in_h, model_config.in_w, keypoint_score_threshold,
         prediction.keypoint_affinity)])
    out = []
    for b in range(obj.shape[0]):
        dets = []
        for r in obj[b, :obj_n[b]]:
            label = int(r[0])
            nk = len(object_config.configs[label].keypoints or [])
            dets.append(KeypointDetection(label=label, score=float(r[1]), y=float(r[2]), x=float(r[3]),
                                          h=float(r[4]), w=float(r[5]),
                                          depth=float(r[6]) if prediction.depth is not None else None,
                                          keypoints=[None] * nk, keypoint_scores=[None] * nk,
                                          keypoint_affinities=[None] * nk, cam_t_object=None))
        for r in kp[b, :kp_n[b]]:
            obj_index, slot = object_config.decode_keypoint_index(int(r[0]))
            cands = [d for d in dets if d.label == obj_index and d.keypoints[slot] is None]
            if not cands:
                continue
            ky, kx = float(r[2]), float(r[3])
            ay, ax = float(r[8]), float(r[9])
            ang = atan2(ay, ax)
            errs = [abs(ang - atan2(ky - d.y, kx - d.x)) for d in cands]
            best = cands[errs.index(min(errs))]
            best.keypoints[slot] = (ky, kx)
            best.keypoint_affinities[slot] = (ay, ax)
            best.keypoint_scores[slot] = float(r[1])
        _solve_poses(dets, model_config, object_config, M_projection)
        out.append(dets)
    return out


MAX_SLOTS = 32  # tv_match_keypoints keeps an object's taken slots in one 32-bit mask


class KeypointRecords(NamedTuple):
    """What decode_keypoints computes, as arrays: `records` [B, K, 10] / `counts` [B] of the objects and
    `keypoint_records` [B, K_kp, 10] / `keypoint_counts` [B] of the keypoints (tv_decode mode 1: label,
    score, y, x, h, w, depth, flat index, affinity y, affinity x), `slot_kp` [B, K, max_slots] int32 the
    keypoint rank held by (object, slot) or -1, `n_matched` [B, K] int32, `kp_det` [B, K_kp] int32 the
    object rank a keypoint went to or -1 (the contract: tv_match_keypoints in include/tauv_vision_amd.h)."""
    records: object
    counts: object
    keypoint_records: object
    keypoint_counts: object
    slot_kp: object
    n_matched: object
    kp_det: object


def keypoint_owner_tables(object_config):
    """(owner label, owner slot) int32 lists over the flat keypoint index and the most keypoints any object
    has. ValueError for an object with more than 32 keypoints, or a config without keypoints."""
    n = object_config.n_keypoints
    if n < 1:
        raise ValueError("the object config has no keypoints")
    owners = [object_config.decode_keypoint_index(i) for i in range(n)]
    max_slots = max(len(c.keypoints or []) for c in object_config.configs)
    if max_slots > MAX_SLOTS:
        raise ValueError(f"an object has {max_slots} keypoints; the device matching takes at most {MAX_SLOTS}")
    return [o for o, _ in owners], [s for _, s in owners], max_slots


POSE = 16  # R row-major (9), t (3), valid, n points, rms reprojection error in pixels, LM iterations


def pose_model_points(object_config) -> np.ndarray:
    """float32 [n_labels, max_slots, 3]: every object's keypoints in its own frame (ObjectConfig.keypoints),
    NaN past an object's keypoints and for an object without keypoints: tv_solve_poses' `model_points`."""
    _, _, S = keypoint_owner_tables(object_config)
    out = np.full((object_config.n_labels, S, 3), np.nan, dtype=np.float32)
    for c, cfg in enumerate(object_config.configs):
        for s, k in enumerate(cfg.keypoints or []):
            out[c, s] = k
    return out


def camera_of(M_projection):
    """(fx, fy, cx, cy) of a projection matrix (at least 2 x 3; the node's has a zero last row)."""
    M = np.asarray(M_projection, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] < 2 or M.shape[1] < 3:
        raise ValueError(f"M_projection must be at least 2 x 3, got {list(M.shape)}")
    return float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2])


class DevicePoseSolver:
    """Static-buffer object poses from matched keypoints (tv_solve_poses, csrc/pose.hip): the reference's
    solvePnP stage (decode.py:137-172) for every detection of a DeviceKeypointDecoder in one launch on the
    current stream, with no allocation and no host synchronisation, so decode + match + solve can be
    captured in one HIP graph. Holds `model_points` (pose_model_points) on the device and `poses`
    [B, K, 16] fp32 (R row-major, t, valid, n, rms pixels, LM iterations; NaN in R, t, rms where not valid)
    - `out`: a caller-owned contiguous buffer for it (a DeviceKeypointDecoder's `poses` section). Every
    element is overwritten by every call. The pose is the minimiser of the pixel reprojection error
    (include/tauv_vision_amd.h); parity with OpenCV's iteration is not claimed."""

    def __init__(self, B, K, K_kp, object_config, device, out=None):
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DevicePoseSolver needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if int(B) < 0 or not 1 <= int(K) <= 256 or not 1 <= int(K_kp) <= 1024:
            raise ValueError(f"DevicePoseSolver needs B >= 0, K in 1..256 and K_kp in 1..1024, got {B}, {K}, {K_kp}")
        self.B, self.K, self.K_kp = int(B), int(K), int(K_kp)
        table = pose_model_points(object_config)
        self.n_labels, self.max_slots = table.shape[:2]
        self.model_points = torch.from_numpy(table).to(self.device)
        self.poses = _lib.check_out(out, (self.B, self.K, POSE), self.device, "DevicePoseSolver")

    def __call__(self, records, counts, keypoint_records, keypoint_counts, slot_kp, model_config, camera,
                 min_points=6):
        """records [B, K, 10] / counts [B], keypoint_records [B, K_kp, 10] / keypoint_counts [B], slot_kp
        [B, K, max_slots] on the device (DeviceKeypointDecoder's), camera = (fx, fy, cx, cy). Returns the
        device `poses`. ValueError before the launch for host tensors, other shapes or types than the
        solver's, a camera that is not four numbers with finite non-zero fx, fy, min_points outside 6..32."""
        from .localize import _check_camera, _check_counts, _require
        B, K, K_kp, S = self.B, self.K, self.K_kp, self.max_slots
        for name, t, shape in (("records", records, (B, K, REC)), ("keypoint_records", keypoint_records, (B, K_kp, REC))):
            _require(t, name, torch.float32, self.device)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        _check_counts(counts, B, self.device)
        _check_counts(keypoint_counts, B, self.device)
        _require(slot_kp, "slot_kp", torch.int32, self.device)
        if tuple(slot_kp.shape) != (B, K, S):
            raise ValueError(f"slot_kp must be {[B, K, S]}, got {list(slot_kp.shape)}")
        if camera is None or len(camera) != 4:
            raise ValueError(f"camera must be (fx, fy, cx, cy), got {camera}")
        fx, fy, cx, cy = (float(v) for v in camera)
        _check_camera(fx, fy)
        if not (np.isfinite(fx) and np.isfinite(fy)):
            raise ValueError("fx and fy must be finite")
        if not 6 <= int(min_points) <= 32:
            raise ValueError(f"min_points must be in 6..32, got {min_points}")
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().tv_solve_poses(
            vp(records), vp(counts), vp(keypoint_records), vp(keypoint_counts), vp(slot_kp), vp(self.model_points),
            self.n_labels, S, B, K, K_kp, int(model_config.in_h), int(model_config.in_w), fx, fy, cx, cy,
            int(min_points), vp(self.poses), _lib.stream_of(self.device)), "solve_poses")
        return self.poses


class DeviceKeypointDecoder:
    """Static-buffer decode_keypoints without the host: the object decode, the keypoint decode and the
    matching (tv_match_keypoints, csrc/keypoints.hip) launched on the current stream into preallocated
    device buffers, with no allocation and no host synchronisation — so forward + decode + localisation
    can be captured in one HIP graph. For a fixed (B, C labels, C_kp keypoint channels, H, W, K, K_kp)
    and object config. `records`, `counts`, `keypoint_records`, `keypoint_counts`, `slot_kp`, `n_matched`
    and `kp_det` (KeypointRecords' fields) are views of one allocation `packed`: one copy carries
    everything. Every element is overwritten by every call.
    poses=True appends a `poses` section [B, K, 16] fp32 to `packed`, after `kp_det` (the prefix layout is
    the same either way), which solve() fills (DevicePoseSolver, tv_solve_poses); host_poses() is its
    host view. A call itself never touches it."""

    def __init__(self, B, C, C_kp, H, W, K, K_kp, object_config, device, poses=False):
        owner_label, owner_slot, S = keypoint_owner_tables(object_config)
        if C != object_config.n_labels or C_kp != len(owner_label):
            raise ValueError(f"the object config has {object_config.n_labels} labels and {len(owner_label)} keypoints, "
                             f"the decoder {C} and {C_kp} channels")
        if not 1 <= K <= 256 or not 1 <= K_kp <= 1024:
            raise ValueError(f"the device matching takes 1..256 objects and 1..1024 keypoints per image, got {K}, {K_kp}")
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceKeypointDecoder needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.shape = (B, C, C_kp, H, W, K, K_kp)
        self.max_slots = S
        self.objects = DeviceDecoder(B, C, H, W, K, dev)
        self.keypoints = DeviceDecoder(B, C_kp, H, W, K_kp, dev)
        self.owner_label = torch.tensor(owner_label, dtype=torch.int32).to(dev)
        self.owner_slot = torch.tensor(owner_slot, dtype=torch.int32).to(dev)
        sizes = [B * K * REC, B, B * K_kp * REC, B, B * K * S, B * K, B * K_kp]  # 4-byte elements
        npose = B * K * POSE if poses else 0
        self.packed = torch.zeros((sum(sizes) + npose) * 4, dtype=torch.uint8, device=dev)
        self._offsets = [sum(sizes[:i]) * 4 for i in range(len(sizes) + 1)]
        self.poses = self.pose_solver = None
        if poses:
            self.poses = self.packed[self._offsets[-1]:].view(torch.float32).view(B, K, POSE)
            self.pose_solver = DevicePoseSolver(B, K, K_kp, object_config, dev, out=self.poses)
        self.records, self.counts, self.keypoint_records, self.keypoint_counts, self.slot_kp, self.n_matched, \
            self.kp_det = self._views(self.packed)
        # the two decodes write straight into `packed`
        self.objects.packed, self.objects.records, self.objects.counts = None, self.records, self.counts
        self.keypoints.packed, self.keypoints.records, self.keypoints.counts = \
            None, self.keypoint_records, self.keypoint_counts
        self._host = None

    def _views(self, buf):
        B, _, _, _, _, K, K_kp = self.shape
        o = self._offsets
        f32 = lambda i, *shape: buf[o[i]:o[i + 1]].view(torch.float32).view(*shape)
        i32 = lambda i, *shape: buf[o[i]:o[i + 1]].view(torch.int32).view(*shape)
        return KeypointRecords(f32(0, B, K, REC), i32(1, B), f32(2, B, K_kp, REC), i32(3, B),
                               i32(4, B, K, self.max_slots), i32(5, B, K), i32(6, B, K_kp))

    def _check(self, prediction):
        B, C, C_kp, H, W, _, _ = self.shape
        if prediction.keypoint_heatmap is None or prediction.keypoint_affinity is None:
            raise ValueError("the prediction has no keypoint heads (keypoint_heatmap / keypoint_affinity are None)")
        want = (("heatmap", prediction.heatmap, (B, C, H, W)), ("keypoint_heatmap", prediction.keypoint_heatmap,
                                                                (B, C_kp, H, W)),
                ("keypoint_affinity", prediction.keypoint_affinity, (B, C_kp, 2, H, W)),
                ("size", prediction.size, (B, H, W, 2)), ("depth", prediction.depth, (B, H, W, 1)))
        for name, t, shape in want:
            if t is None and name == "depth":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{name} must be a float32 tensor")
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the decoder on {self.device}")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} shape {tuple(t.shape)} != decoder shape {shape}")

    def __call__(self, prediction, model_config, score_threshold, keypoint_score_threshold) -> KeypointRecords:
        """The three launches on the current stream; returns the device views. Refuses (ValueError, before
        any launch) a prediction without keypoint heads, host tensors and shapes other than the decoder's."""
        self._check(prediction)
        mc = model_config
        self.objects(prediction.heatmap, prediction.size, None, prediction.depth, 1, mc.downsample_ratio, mc.in_h,
                     mc.in_w, score_threshold)
        self.keypoints(prediction.keypoint_heatmap, prediction.size, None, None, 1, mc.downsample_ratio, mc.in_h,
                       mc.in_w, keypoint_score_threshold, prediction.keypoint_affinity)
        return self.match()

    def match(self) -> KeypointRecords:
        """The matching alone, on the records and counts the buffers hold (the last launch of a call)."""
        B, _, C_kp, _, _, K, K_kp = self.shape
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().tv_match_keypoints(
            vp(self.records), vp(self.counts), vp(self.keypoint_records), vp(self.keypoint_counts),
            vp(self.owner_label), vp(self.owner_slot), C_kp, self.max_slots, B, K, K_kp, vp(self.kp_det),
            vp(self.slot_kp), vp(self.n_matched), _lib.stream_of(self.device)), "match_keypoints")
        return KeypointRecords(self.records, self.counts, self.keypoint_records, self.keypoint_counts, self.slot_kp,
                               self.n_matched, self.kp_det)

    def solve(self, model_config, camera, min_points=6):
        """The poses of the detections the buffers hold (one launch after match()): the device `poses`
        [B, K, 16]. camera = (fx, fy, cx, cy). A decoder built with poses=True only."""
        if self.pose_solver is None:
            raise ValueError("DeviceKeypointDecoder.solve needs a decoder built with poses=True")
        return self.pose_solver(self.records, self.counts, self.keypoint_records, self.keypoint_counts, self.slot_kp,
                                model_config, camera, min_points)

    def host(self) -> KeypointRecords:
        """The last call's arrays on the host: `packed` copied to pinned memory, one synchronisation. The
        tensors are views of the decoder's pinned mirror, overwritten by the next host()."""
        if self._host is None:
            self._host = torch.empty(self.packed.numel(), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.device(self.device):
            self._host.copy_(self.packed, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        return self._views(self._host)

    def host_poses(self):
        """`poses` [B, K, 16] of the last host(): a view of the same pinned mirror (no copy, no
        synchronisation of its own). A decoder built with poses=True, after a host()."""
        if self.poses is None or self._host is None:
            raise ValueError("host_poses needs a decoder built with poses=True and a host() before it")
        return self._host[self._offsets[-1]:].view(torch.float32).view(tuple(self.poses.shape))


_KP_DECODERS = {}  # (device, shape, owner tables) -> DeviceKeypointDecoder; under _DECODERS_LOCK


def decode_keypoints_records(prediction, model_config, object_config, n_detections: int,
                             keypoint_n_detections: int, score_threshold: float,
                             keypoint_score_threshold: float) -> KeypointRecords:
    """decode_keypoints() with the matching on the device and without the per-detection Python objects
    (the keypoint analogue of decode_records): KeypointRecords of host numpy arrays — three launches, one
    D2H copy, one host synchronisation. The prediction must be on the GPU."""
    return _keypoints_records(prediction, model_config, object_config, n_detections, keypoint_n_detections,
                              score_threshold, keypoint_score_threshold, None, 6)


def decode_keypoint_poses(prediction, model_config, object_config, M_projection, n_detections: int,
                          keypoint_n_detections: int, score_threshold: float, keypoint_score_threshold: float,
                          min_points: int = 6):
    """decode_keypoints_records() plus the pose of every object with at least min_points matched
    keypoints: (KeypointRecords of host numpy arrays, poses [B, K, 16] float32: R row-major, t, valid, n,
    rms pixels, LM iterations). Four launches (two decodes, tv_match_keypoints, tv_solve_poses), one D2H
    copy, one host synchronisation. M_projection: fx, fy, cx, cy = M[0,0], M[1,1], M[0,2], M[1,2]."""
    return _keypoints_records(prediction, model_config, object_config, n_detections, keypoint_n_detections,
                              score_threshold, keypoint_score_threshold, camera_of(M_projection), min_points)


def _keypoints_records(prediction, model_config, object_config, n_detections, keypoint_n_detections, score_threshold,
                       keypoint_score_threshold, camera, min_points):
    """decode_keypoints_records (camera None) / decode_keypoint_poses through the cached decoder of the shape."""
    owner_label, owner_slot, _ = keypoint_owner_tables(object_config)
    heat = prediction.heatmap
    if not isinstance(heat, torch.Tensor) or not heat.is_cuda:
        raise ValueError("the prediction must be on the GPU")
    if prediction.keypoint_heatmap is None or prediction.keypoint_affinity is None:
        raise ValueError("the prediction has no keypoint heads (keypoint_heatmap / keypoint_affinity are None)")
    B, C, H, W = heat.shape
    _empty_batch_check(B)
    C_kp = prediction.keypoint_heatmap.shape[1]
    table = None if camera is None else pose_model_points(object_config).tobytes()
    key = (heat.device.index, B, C, C_kp, H, W, int(n_detections), int(keypoint_n_detections), tuple(owner_label),
           tuple(owner_slot), table)
    with _DECODERS_LOCK:
        dec = _KP_DECODERS.get(key)
        if dec is None:
            if len(_KP_DECODERS) >= _DECODERS_MAX:
                _KP_DECODERS.pop(next(iter(_KP_DECODERS)))
            dec = DeviceKeypointDecoder(B, C, C_kp, H, W, int(n_detections), int(keypoint_n_detections), object_config,
                                        heat.device, poses=camera is not None)
            _KP_DECODERS[key] = dec
        with torch.cuda.device(heat.device):
            dec(prediction, model_config, score_threshold, keypoint_score_threshold)
            if camera is None:
                return KeypointRecords(*[t.numpy().copy() for t in dec.host()])
            dec.solve(model_config, camera, min_points)
            rec = KeypointRecords(*[t.numpy().copy() for t in dec.host()])
            return rec, dec.host_poses().numpy().copy()


def keypoint_detections_from_records(records, counts, keypoint_records, slot_kp, has_depth, model_config,
                                     object_config, M_projection, poses=None) -> List[List[KeypointDetection]]:
    """The [[KeypointDetection]] of decode_keypoints() from KeypointRecords' host arrays (numpy or host
    tensors), then the host PnP (_solve_poses) as there. poses [B, K, 16] (tv_solve_poses' rows on the host,
    numpy or a host tensor): cam_t_object = (R float64 [3, 3], t float64 [3, 1]) - the tuple _solve_poses
    stores - from the valid rows instead, None elsewhere; _solve_poses is not called."""
    records, counts, keypoint_records, slot_kp = (np.asarray(a) for a in (records, counts, keypoint_records, slot_kp))
    if poses is not None:
        poses = np.asarray(poses)
        if poses.shape != records.shape[:2] + (POSE,):
            raise ValueError(f"poses must be {list(records.shape[:2]) + [POSE]}, got {list(poses.shape)}")
    out = []
    for b in range(records.shape[0]):
        dets = []
        for d, r in enumerate(records[b, :counts[b]]):
            label = int(r[0])
            nk = len(object_config.configs[label].keypoints or [])
            kps = [keypoint_records[b, k] if k >= 0 else None for k in slot_kp[b, d, :nk]]
            dets.append(KeypointDetection(
                label=label, score=float(r[1]), y=float(r[2]), x=float(r[3]), h=float(r[4]), w=float(r[5]),
                depth=float(r[6]) if has_depth else None,
                keypoints=[None if q is None else (float(q[2]), float(q[3])) for q in kps],
                keypoint_scores=[None if q is None else float(q[1]) for q in kps],
                keypoint_affinities=[None if q is None else (float(q[8]), float(q[9])) for q in kps],
                cam_t_object=None))
            if poses is not None and poses[b, d, 12] == 1:
                row = poses[b, d].astype(np.float64)
                dets[-1].cam_t_object = (row[0:9].reshape(3, 3), row[9:12].reshape(3, 1))
        if poses is None:
            _solve_poses(dets, model_config, object_config, M_projection)
        out.append(dets)
    return out


def _solve_poses(dets, model_config, object_config, M_projection):
    """decode.py:137-172: PnP for detections with >= 6 matched keypoints (needs OpenCV).
    The reference stores the pose on its last matched detection variable (decode.py:172);
    here it is stored on the detection being solved."""
    for d in dets:
        pts = [(i, k) for i, k in enumerate(d.keypoints) if k is not None]
        if len(pts) < 6:
            continue
        try:
            import cv2
        except ImportError as e:
            raise RuntimeError("decode_keypoints: >= 6 keypoints matched; solvePnP needs OpenCV (cv2)") from e
        img_pts = np.array([[k[1] * model_config.in_w, k[0] * model_config.in_h] for _, k in pts])
        obj_pts = np.array([object_config.configs[d.label].keypoints[i] for i, _ in pts])
        ok, rvec, tvec = cv2.solvePnP(obj_pts, img_pts, M_projection, None, cv2.SOLVEPNP_ITERATIVE)
        if ok:
            rot, _ = cv2.Rodrigues(rvec)
            d.cam_t_object = (rot, tvec)


def angle_get_bins(bin_overlap: float):
    """decode.py:282-288."""
    return ((pi / 2, -bin_overlap / 2, pi + bin_overlap / 2), (-pi / 2, -pi - bin_overlap / 2, bin_overlap / 2))


def angle_decode(predicted_bin: torch.Tensor, predicted_offset: torch.Tensor, theta_range: float,
                 bin_overlap: float) -> torch.Tensor:
    """decode.py:291-316 (not wired into decode() in the reference either)."""
    (c0, _, _), (c1, _, _) = angle_get_bins(bin_overlap)
    p0 = torch.softmax(predicted_bin[..., 0:2], dim=-1)[..., 1]
    p1 = torch.softmax(predicted_bin[..., 2:4], dim=-1)[..., 1]
    a0 = c0 + torch.atan2(predicted_offset[..., 0], predicted_offset[..., 1])
    a1 = c1 + torch.atan2(predicted_offset[..., 2], predicted_offset[..., 3])
    ang = torch.where(p1 > p0, a1, a0) % (2 * pi)
    return ang * (theta_range / (2 * pi))


def depth_decode(prediction: torch.Tensor) -> torch.Tensor:
    """decode.py:319-324."""
    return (1 / torch.sigmoid(prediction)) - 1
