"""Evaluation of a trained detector on the GPU: the precision / recall and the precision-recall curve of
the reference's centernet/scripts/evaluate.py and evaluate_keypoints.py, in ONE pass over the data set
(csrc/evaluate.hip; the contract is tv_evaluate_detections' in include/tauv_vision_amd.h).

The reference's evaluate_precision_recall_curve runs the whole data set once per score threshold (ten
times), builds a Python Detection per record with a device sync per scalar, and matches detections to
truths in nested Python loops on the CPU. Its detections at threshold t are the top-K records with
score >= t, and its matching walks them in descending score; the walk at t is therefore a prefix of the
walk at the lowest threshold, a record's match depends only on the records before it, and one walk gives
every record a true-positive flag. n_tp(t) and n_detections(t) are counts over score >= t. Per batch:
the native forward, one DeviceDecoder call at K = 100 and the lowest threshold, one evaluation launch;
nothing is copied to the host until the data set ends (DeviceEvaluator.result: one copy).

In the reference's evaluate.py, replace its two functions by
    from tauv_vision_amd.evaluate import evaluate_precision_recall, evaluate_precision_recall_curve
(the curve returns (precision, recall) instead of plotting).

Reproduced as they are: the walk order (descending score, the later record first among equal scores),
first qualifying truth wins (not the best IoU), iou_threshold = 0 lets every pair of equal labels pass
(disjoint boxes too), precision = 1 without detections, ZeroDivisionError without truths, and the stop
after 101 batches (`max_batches`; None: the whole loader).

Differences from the reference:
  * the match tests are evaluated in double on the fp32 values; the reference mixes Python floats with
    fp32 0-d tensors, which moves an IoU or a distance by about 1e-7 relative: a pair that close to the
    threshold may fall on the other side;
  * a NaN score (the reference's sigmoid gives none) passes no threshold and walks last;
  * batches must go to a GPU (the reference's script forces the CPU);
  * at most 256 truths per image, 1024 records per image and 64 thresholds.
"""
import ctypes
from itertools import islice
from typing import NamedTuple

import torch

from . import _lib
from .decode import REC, DeviceDecoder
from .localize import _check_counts, _require

BOX, CENTRE = 0, 1
MAX_K, MAX_N, MAX_T = 1024, 256, 64  # csrc/evaluate.hip
N_DETECTIONS = 100  # the reference's decode(prediction, model_config, 100, score_threshold)


class EvaluationResult(NamedTuple):
    """precision [T], recall [T] float64; n_tp [T], n_detections [T] int64 (host tensors); n_truth int."""
    precision: object
    recall: object
    n_tp: object
    n_detections: object
    n_truth: int


def _mode(mode):
    if mode in (BOX, "box"):
        return BOX
    if mode in (CENTRE, "centre", "center"):
        return CENTRE
    raise ValueError(f"mode must be 0 / 'box' or 1 / 'centre', got {mode!r}")


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class DeviceEvaluator:
    """Static-buffer evaluation for up to B images of K records and N truths each: `update` launches one
    kernel on the current stream that matches the batch's records to its truths and ADDS the batch's counts
    to `totals` [2T + 1] int64 on the device (n_tp[T], n_detections[T], n_truth), with no allocation and no
    host synchronisation, so forward -> DeviceDecoder -> update captures in one HIP graph. `det_truth`
    [B, K] int32 holds the truth index every record of the last batch took, or -1. `result()` makes the
    one device-to-host copy. `columns`: where label, score, y, x, h, w sit in a record (DeviceDecoder's:
    0..5 of 10; detection_records' rows: (1, 3, 4, 5, 6, 7) of 8)."""

    def __init__(self, B, K, N, score_thresholds, mode, match_threshold, device, columns=(0, 1, 2, 3, 4, 5),
                 rec_stride=REC, _totals=None):
        self.mode = _mode(mode)
        thr = torch.as_tensor(score_thresholds, dtype=torch.float32).detach().reshape(-1).cpu()
        B, K, N, rec_stride = int(B), int(K), int(N), int(rec_stride)
        if B < 1:
            raise ValueError(f"B must be >= 1, got {B}")
        if not 1 <= K <= MAX_K or not 1 <= N <= MAX_N or not 1 <= thr.numel() <= MAX_T:
            raise ValueError(f"the device evaluation takes 1..{MAX_K} records and 1..{MAX_N} truths per image and "
                             f"1..{MAX_T} score thresholds, got {K}, {N}, {thr.numel()}")
        columns = tuple(int(c) for c in columns)
        if len(columns) != 6 or rec_stride < 1 or any(not 0 <= c < rec_stride for c in columns):
            raise ValueError(f"columns must be the 6 columns of label, score, y, x, h, w inside a record of "
                             f"{rec_stride}, got {columns}")
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceEvaluator needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.B, self.K, self.N, self.T = B, K, N, thr.numel()
        self.columns, self.rec_stride = columns, rec_stride
        self.match_threshold = float(match_threshold)
        self._cols = (_lib.c_i32 * 6)(*columns)
        self._host_thresholds = thr  # (grown() builds from these: no device-to-host copy in mid data set)
        self.score_thresholds = thr.to(dev)
        # truths that do not arrive as the kernel reads them are staged here, padded as invalid
        self.valid = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        self.label = torch.zeros((B, N), dtype=torch.int64, device=dev)
        self.center = torch.zeros((B, N, 2), dtype=torch.float32, device=dev)
        self.size = torch.zeros((B, N, 2), dtype=torch.float32, device=dev)
        self.det_truth = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        if _totals is None:
            _totals = torch.zeros(2 * self.T + 1, dtype=torch.int64, device=dev)
        self.totals = _totals

    def grown(self, B, N):
        """An evaluator for at least B images and N truths per image that goes on adding to the same totals."""
        return DeviceEvaluator(max(B, self.B), self.K, max(N, self.N), self._host_thresholds, self.mode,
                               self.match_threshold, self.device, self.columns, self.rec_stride, _totals=self.totals)

    def reset(self):
        self.totals.zero_()

    def _direct(self, t, dtypes, shape):
        return isinstance(t, torch.Tensor) and t.dtype in dtypes and t.device == self.device and t.is_contiguous() \
            and tuple(t.shape) == shape

    def _truths(self, batch, valid, label, center, size):
        """(valid, label, center, size, n): the caller's tensors where the kernel can read them as they are
        (on the device, bool / uint8, int64, fp32, contiguous, exactly `batch` images), else the static
        buffers filled from them, with the images' missing truths invalid."""
        need_size = self.mode == BOX
        if size is None and need_size:
            raise ValueError("box mode needs the truths' size")
        tensors = (("valid", valid), ("label", label), ("center", center)) + ((("size", size),) if need_size else ())
        for name, t in tensors:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if valid.dim() != 2 or valid.shape[0] != batch:
            raise ValueError(f"valid must be [{batch}, n], got {list(valid.shape)}")
        n = valid.shape[1]
        if n > self.N:
            raise ValueError(f"{n} truths per image, the evaluator takes {self.N}")
        for name, t, shape in (("label", label, (batch, n)), ("center", center, (batch, n, 2))) + \
                ((("size", size, (batch, n, 2)),) if need_size else ()):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        if n >= 1 and self._direct(valid, (torch.bool, torch.uint8), (batch, n)) \
                and self._direct(label, (torch.int64,), (batch, n)) \
                and self._direct(center, (torch.float32,), (batch, n, 2)) \
                and (not need_size or self._direct(size, (torch.float32,), (batch, n, 2))):
            return valid, label, center, size if need_size else None, n
        self.valid.zero_()
        if n:
            self.valid[:batch, :n].copy_(valid.to(torch.bool), non_blocking=True)
            self.label[:batch, :n].copy_(label, non_blocking=True)
            self.center[:batch, :n].copy_(center, non_blocking=True)
            if need_size:
                self.size[:batch, :n].copy_(size, non_blocking=True)
        return self.valid, self.label, self.center, self.size if need_size else None, self.N

    def update(self, records, counts, valid, label, center, size=None, batch=None):
        """Add one batch: records [>= batch, K, rec_stride] fp32 and counts [>= batch] int32 on the device
        (DeviceDecoder's buffers as they are), the truths valid [batch, n] bool, label [batch, n] int64,
        center [batch, n, 2] (y, x), size [batch, n, 2] (h, w; unused in centre mode) with n <= N. `batch`
        (default: all the records' images) may be smaller than B: the last batch of a loader. One launch on
        the current stream when the truths are device tensors of those types; no synchronisation. ValueError
        before any launch otherwise. Returns det_truth[:batch]."""
        _require(records, "records", torch.float32, self.device)
        if records.dim() != 3 or tuple(records.shape[1:]) != (self.K, self.rec_stride):
            raise ValueError(f"records must be [batch, {self.K}, {self.rec_stride}], got {list(records.shape)}")
        batch = records.shape[0] if batch is None else int(batch)
        if not 1 <= batch <= min(self.B, records.shape[0]):
            raise ValueError(f"batch must be in 1..{min(self.B, records.shape[0])} (the evaluator's B and the records' "
                             f"images), got {batch}")
        _check_counts(counts[:batch] if isinstance(counts, torch.Tensor) and counts.dim() == 1 else counts, batch,
                      self.device)
        v, l, c, s, n = self._truths(batch, valid, label, center, size)
        _lib.check(_lib.lib().tv_evaluate_detections(
            _vp(records), self.rec_stride, _vp(counts), self._cols, batch, self.K, _vp(v), _vp(l), _vp(c), _vp(s), n,
            self.mode, self.match_threshold, _vp(self.score_thresholds), self.T, _vp(self.det_truth),
            _vp(self.totals), _lib.stream_of(self.device)), "evaluate_detections")
        return self.det_truth[:batch]

    def result(self) -> EvaluationResult:
        """The data set's counts (ONE device-to-host copy, which waits for the launches so far) and the
        reference's precision = n_tp / n_detections if n_detections > 0 else 1, recall = n_tp / n_truth per
        threshold — ZeroDivisionError without a truth, as there (evaluate.py:205-206)."""
        host = self.totals.cpu()
        T = self.T
        n_tp, n_det, n_truth = host[:T].clone(), host[T:2 * T].clone(), int(host[2 * T])
        precision = [int(a) / int(b) if int(b) > 0 else 1 for a, b in zip(n_tp, n_det)]
        recall = [int(a) / n_truth for a in n_tp]
        return EvaluationResult(torch.tensor(precision, dtype=torch.float64), torch.tensor(recall, dtype=torch.float64),
                                n_tp, n_det, n_truth)


def _evaluate(centernet, model_config, data_loader, device, score_thresholds, mode, match_threshold, max_batches):
    """One pass over the loader: per batch the native forward, one decode at the lowest threshold, one
    evaluation launch. Returns the EvaluationResult."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the evaluation runs on the GPU, got device {device}")
    thr = torch.as_tensor(score_thresholds, dtype=torch.float32).detach().reshape(-1).cpu()
    if not 1 <= thr.numel() <= MAX_T:
        raise ValueError(f"1..{MAX_T} score thresholds, got {thr.numel()}")
    lowest = float(thr.min())
    mc = model_config
    decoders, evaluator = {}, None
    batches = data_loader if max_batches is None else islice(data_loader, int(max_batches))
    with torch.cuda.device(device):
        for batch in batches:
            batch = batch.to(device)
            with torch.no_grad():
                prediction = centernet.forward(batch.img)
            heat = prediction.heatmap
            shape = tuple(heat.shape)
            if shape not in decoders:
                decoders[shape] = DeviceDecoder(*shape, N_DETECTIONS, heat.device)
            if mode == BOX:  # decode(): offsets and the downsample ratio
                records, counts = decoders[shape](heat, prediction.size, prediction.offset, prediction.depth, 0,
                                                  mc.downsample_ratio, mc.in_h, mc.in_w, lowest)
            else:  # decode_keypoints(): its object records (one detection per record, decode.py:74-98)
                records, counts = decoders[shape](heat, prediction.size, None, prediction.depth, 1,
                                                  mc.downsample_ratio, mc.in_h, mc.in_w, lowest)
            B, N = shape[0], max(int(batch.valid.shape[1]), 1)
            if evaluator is None:
                evaluator = DeviceEvaluator(B, N_DETECTIONS, N, thr, mode, match_threshold, heat.device)
            elif B > evaluator.B or N > evaluator.N:
                evaluator = evaluator.grown(B, N)
            evaluator.update(records, counts, batch.valid, batch.label, batch.center,
                             batch.size if mode == BOX else None, batch=B)
        if evaluator is None:  # an empty loader: the reference divides 0 by 0 truths
            raise ZeroDivisionError("division by zero")
        return evaluator.result()


def evaluate_precision_recall(centernet, model_config, data_loader, device, score_threshold, iou_threshold,
                              max_batches=101):
    """evaluate.py:167-208 -> (precision, recall) Python numbers. `max_batches` is the reference's
    `if batch_i > 100: break` (None: the whole loader). Batches are duck-typed like the loss's truth:
    .to(device), .img, .valid, .label, .center, .size."""
    r = _evaluate(centernet, model_config, data_loader, device, [float(score_threshold)], BOX, iou_threshold,
                  max_batches)
    n_tp, n_det = int(r.n_tp[0]), int(r.n_detections[0])
    return (n_tp / n_det if n_det > 0 else 1, n_tp / r.n_truth)


def evaluate_precision_recall_curve(centernet, model_config, data_loader, device, iou_threshold,
                                    score_thresholds=None, max_batches=101):
    """evaluate.py:211-233 without the plot -> (precision [T], recall [T]) float64 tensors, from ONE pass over
    the loader (the reference makes one per threshold). Default thresholds: torch.linspace(0, 1, 10)."""
    if score_thresholds is None:
        score_thresholds = torch.linspace(0, 1, 10)
    r = _evaluate(centernet, model_config, data_loader, device, score_thresholds, BOX, iou_threshold, max_batches)
    return r.precision, r.recall


def evaluate_keypoints_precision_recall(centernet, model_config, object_config, M_projection, data_loader, device,
                                        score_threshold, keypoint_score_threshold, keypoint_angle_threshold,
                                        distance_threshold, max_batches=101):
    """evaluate_keypoints.py:104-158 -> (precision, recall): a detection and a truth of one label match
    unless their centres are farther apart than `distance_threshold`. decode_keypoints makes one detection
    per object record at or above `score_threshold` (decode.py:74-98) and its keypoint matching changes
    neither their number nor their label, score, y, x, so `object_config`, `M_projection`,
    `keypoint_score_threshold` and `keypoint_angle_threshold` do not enter the counts: they are taken for
    the reference's signature and ignored."""
    r = _evaluate(centernet, model_config, data_loader, device, [float(score_threshold)], CENTRE, distance_threshold,
                  max_batches)
    n_tp, n_det = int(r.n_tp[0]), int(r.n_detections[0])
    return (n_tp / n_det if n_det > 0 else 1, n_tp / r.n_truth)


def evaluate_keypoints_precision_recall_curve(centernet, model_config, object_config, M_projection, data_loader,
                                              device, keypoint_score_threshold, keypoint_angle_threshold,
                                              distance_threshold, score_thresholds=None, max_batches=101):
    """evaluate_keypoints.py:161-183 without the plot -> (precision [T], recall [T]) from one pass. Default
    thresholds: torch.linspace(0.9, 1, 10). The keypoint arguments are ignored (see
    evaluate_keypoints_precision_recall)."""
    if score_thresholds is None:
        score_thresholds = torch.linspace(0.9, 1, 10)
    r = _evaluate(centernet, model_config, data_loader, device, score_thresholds, CENTRE, distance_threshold,
                  max_batches)
    return r.precision, r.recall
