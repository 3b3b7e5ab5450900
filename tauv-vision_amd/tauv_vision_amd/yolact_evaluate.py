"""Evaluation of a trained YOLACT on the GPU: box and mask average precision at IoU 0.50:0.05:0.95 in one
pass over the data set (csrc/yolact_eval.hip; the contracts are tv_yolact_mask_overlap's and
tv_yolact_evaluate_match's in include/tauv_vision_amd.h).

The reference measures a trained YOLACT by its validation loss only (yolact/scripts/train.py:314-358, and
picks the "best" checkpoint by it, :499-501); its evaluate.py stops at `# TODO: Implement NMS`. This module
gives the figure an instance-segmentation model is chosen by. Per batch: the native forward through a
YolactDetector with frame_masks="bilinear" at (in_h, in_w) — the binarised masks of evaluate_batch.py:98-102
as packed bits —, one detection_records call for the softmax rows, and DeviceYolactEvaluator.update: the
K x N pixel intersections from the bits and the ONE seg map of the sample (pixel value i means truth i,
segmentation_dataset.py:97-100, so the truth masks are disjoint; 254 is invalid image), then the matching
for both kinds and every threshold. Every record's score, label and true-positive bits go to a log on the
device; nothing reaches the host until result(), which makes ONE copy. In run_validation_epoch this is

    evaluation = evaluate_average_precision(model, val_loader, device)

The rules (each also in the header):
  * a detection's label is 1 + argmax over the foreground columns of its softmax row, its score that
    probability; the background column never names a detection;
  * detections walk in descending score, the lower record index first among equal scores;
  * per kind and threshold a detection takes the free truth of its label with the LARGEST IoU >= the
    threshold, the lowest truth index on a tie (tv_evaluate_detections takes the first: not reused);
  * AP is the 101-point interpolated average precision per class; a class without truths is NaN and
    left out of every mean.
"""
import ctypes
from itertools import islice
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

MAX_K, MAX_N, MAX_T, MAX_C = 256, 64, 16, 254  # csrc/yolact_eval.hip
INVALID_PIXEL = 254
BOX, MASK = 0, 1
_FIRST_CAPACITY = 256  # images the log holds before it first grows


def default_iou_thresholds():
    return torch.linspace(0.5, 0.95, 10).to(torch.float32)


class YolactEvaluation(NamedTuple):
    """ap [2, T, C+1] float64 (kind 0 box, 1 mask; NaN for a class without truths, column 0 always), map [2]
    the mean over thresholds and classes with truths, ap50 / ap75 [2] the means over those classes at the
    threshold nearest 0.5 / 0.75 (NaN when no threshold is within 1e-6 of it), n_truth [C+1] int64,
    n_detections int, and the log sorted by descending score (stable in image, record order): score
    float32, label int32, tp uint32 (bit j box, bit 16 + j mask, at threshold j)."""
    ap: np.ndarray
    map: np.ndarray
    ap50: np.ndarray
    ap75: np.ndarray
    n_truth: np.ndarray
    n_detections: int
    score: np.ndarray
    label: np.ndarray
    tp: np.ndarray

    def precision_recall(self, score_threshold, iou_index, kind):
        """(precision, recall) over all classes of the detections with score >= score_threshold, at IoU
        threshold `iou_index` of kind 0 / "box" or 1 / "mask". precision is 1 without a detection."""
        kind = {"box": BOX, "mask": MASK}.get(kind, kind)
        if kind not in (BOX, MASK) or not 0 <= int(iou_index) < self.ap.shape[1]:
            raise ValueError(f"kind must be 0 / 'box' or 1 / 'mask' and iou_index in 0..{self.ap.shape[1] - 1}")
        sel = self.score >= np.float32(score_threshold)
        n_det = int(sel.sum())
        n_tp = int(((self.tp[sel] >> np.uint32(16 * kind + int(iou_index))) & np.uint32(1)).sum())
        return (n_tp / n_det if n_det > 0 else 1, n_tp / int(self.n_truth.sum()))


def average_precision(log, n_truth, T, iou_thresholds=None) -> YolactEvaluation:
    """The average precision of a detection log, a pure host function in float64 (no library, no GPU).
    log: [images, K, 4] 32-bit words (tv_yolact_evaluate_match's: score as fp32, label, tp word, 1 for a
    detection), numpy or torch; n_truth [C+1] truths per label; T thresholds. iou_thresholds [T] (None: the
    default ten when T == 10) only names the ap50 / ap75 columns.
    Per kind, threshold and class with truths: the class's rows by descending score (stable), cumulative
    tp, precision = ctp / (ctp + cfp), recall = ctp / n_truth, the precision envelope made monotone from
    the right, sampled at np.linspace(0, 1, 101) with searchsorted(recall, r, side="left") (0 past the
    end); AP is the mean of the 101 samples. ZeroDivisionError without any truth; ValueError for a NaN score."""
    if isinstance(log, torch.Tensor):
        log = log.detach().cpu().contiguous().view(torch.int32).numpy()
    words = np.ascontiguousarray(log).view(np.uint32).reshape(-1, 4)
    n_truth = np.asarray(n_truth, dtype=np.int64).reshape(-1)
    T = int(T)
    if not 1 <= T <= MAX_T or n_truth.size < 2:
        raise ValueError(f"need 1..{MAX_T} thresholds and n_truth [C+1] with C >= 1")
    if int(n_truth.sum()) == 0:
        raise ZeroDivisionError("division by zero")
    rows = words[words[:, 3] == 1]
    score = rows[:, 0].copy().view(np.float32)
    label = rows[:, 1].copy().view(np.int32)
    tp = rows[:, 2].copy()
    if np.isnan(score).any():
        raise ValueError("a logged score is NaN")
    order = np.argsort(-score.astype(np.float64), kind="stable")
    score, label, tp = score[order], label[order], tp[order]
    C1 = n_truth.size
    ap = np.full((2, T, C1), np.nan, dtype=np.float64)
    samples = np.linspace(0, 1, 101)
    for c in range(C1):
        if n_truth[c] <= 0:
            continue
        tpc = tp[label == c]
        for kind in (BOX, MASK):
            for j in range(T):
                flags = ((tpc >> np.uint32(16 * kind + j)) & np.uint32(1)).astype(np.float64)
                if flags.size == 0:
                    ap[kind, j, c] = 0.0
                    continue
                ctp = np.cumsum(flags)
                cfp = np.cumsum(1.0 - flags)
                precision = ctp / (ctp + cfp)
                recall = ctp / float(n_truth[c])
                envelope = np.maximum.accumulate(precision[::-1])[::-1]
                at = np.searchsorted(recall, samples, side="left")
                ap[kind, j, c] = np.mean(np.where(at < envelope.size, envelope[np.minimum(at, envelope.size - 1)], 0.0))
    have = n_truth > 0
    if iou_thresholds is None and T == 10:
        iou_thresholds = default_iou_thresholds()
    thr = None if iou_thresholds is None else np.asarray(torch.as_tensor(iou_thresholds, dtype=torch.float32)
                                                         .reshape(-1).numpy(), dtype=np.float64)

    def column(value):
        if thr is None or thr.size != T:
            return np.full(2, np.nan)
        j = int(np.argmin(np.abs(thr - value)))
        if abs(thr[j] - value) > 1e-6:
            return np.full(2, np.nan)
        return np.array([np.mean(np.ascontiguousarray(ap[kind, j, have])) for kind in (BOX, MASK)])
    # (np.mean of a contiguous copy: one summation order, which tests/yolact_eval_ref.py repeats)
    mean = np.array([np.mean(np.ascontiguousarray(ap[kind][:, have])) for kind in (BOX, MASK)])
    return YolactEvaluation(ap, mean, column(0.5), column(0.75), n_truth, int(score.size), score, label, tp)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class DeviceYolactEvaluator:
    """Static-buffer YOLACT evaluation for up to B images of K records and N truths each, C = n_classes
    foreground classes, masks of hw = (H, W). `update` makes two C-ABI calls on the current stream
    (tv_yolact_mask_overlap, tv_yolact_evaluate_match: four launches, the cursor step among them) with no
    host synchronisation, and no allocation unless the log has to grow; `result()` makes the one
    device-to-host copy. The evaluator owns `inter` [B, K, N], `det_area` [B, K], `truth_area` [B, N] and
    `det_truth` [B, K, 2, T] int32 of the last batch (views of its buffers shaped for that batch), and one
    state buffer holding the cursor (images logged so far, int64), the totals (n_truth[C+1], n_bad_label;
    int64) and the log [capacity, K, 4]. The log grows on the host side before a batch could overflow it
    (the host counts the images of its own `update` calls). A captured graph of `update` allocates nothing:
    `reserve(images)` first for every replay to come — the host does not see replays. For a capture the
    truths must be on the direct path (device tensors, bool / uint8, int64, fp32, contiguous, n >= 1): staged
    truths are copied from the caller's tensors inside `update`, and a replay would repeat the copy from the
    tensors of the capture, not read new ones."""

    def __init__(self, B, K, N, n_classes, hw, device, iou_thresholds=None, _capacity=None, _guard_rows=0):
        thr = default_iou_thresholds() if iou_thresholds is None else \
            torch.as_tensor(iou_thresholds, dtype=torch.float32).detach().reshape(-1).cpu()
        B, K, N, C = int(B), int(K), int(N), int(n_classes)
        if B < 1 or len(hw) != 2 or int(hw[0]) < 1 or int(hw[1]) < 1:
            raise ValueError(f"need B >= 1 and hw = (H, W) with H, W >= 1, got {B}, {hw}")
        if not 1 <= K <= MAX_K or not 1 <= N <= MAX_N or not 1 <= C <= MAX_C or not 1 <= thr.numel() <= MAX_T:
            raise ValueError(f"the YOLACT evaluation takes 1..{MAX_K} records and 1..{MAX_N} truths per image, "
                             f"1..{MAX_C} classes and 1..{MAX_T} IoU thresholds, got {K}, {N}, {C}, {thr.numel()}")
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceYolactEvaluator needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.B, self.K, self.N, self.C, self.T = B, K, N, C, thr.numel()
        self.hw = (int(hw[0]), int(hw[1]))
        self._host_thresholds = thr
        self.iou_thresholds = thr.to(dev)
        self.valid = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        self.label = torch.zeros((B, N), dtype=torch.int64, device=dev)
        self.box = torch.zeros((B, N, 4), dtype=torch.float32, device=dev)
        self._inter = torch.zeros(B * K * N, dtype=torch.int32, device=dev)
        self._det_area = torch.zeros(B * K, dtype=torch.int32, device=dev)
        self._truth_area = torch.zeros(B * N, dtype=torch.int32, device=dev)
        self._det_truth = torch.full((B * K * 2 * self.T,), -1, dtype=torch.int32, device=dev)
        self._last = (B, N)
        # state: cursor (2 words), totals (2 (C + 2) words), padding to 16 bytes, log, guard rows
        self._head = (2 + 2 * (C + 2) + 3) // 4 * 4
        self._fixed = _capacity is not None
        self._guard_rows = int(_guard_rows)
        self.capacity = int(_capacity) if self._fixed else _FIRST_CAPACITY
        self._images = 0
        self._state = self._new_state(self.capacity)

    def _new_state(self, capacity):
        words = self._head + (capacity + self._guard_rows) * self.K * 4
        return torch.zeros(words, dtype=torch.int32, device=self.device)

    # views of the state buffer
    @property
    def cursor(self):
        return self._state[:2].view(torch.int64)

    @property
    def totals(self):
        return self._state[2:2 + 2 * (self.C + 2)].view(torch.int64)

    @property
    def log(self):
        return self._state[self._head:self._head + self.capacity * self.K * 4].view(self.capacity, self.K, 4)

    # views of the last batch's outputs
    @property
    def inter(self):
        b, n = self._last
        return self._inter[:b * self.K * n].view(b, self.K, n)

    @property
    def det_area(self):
        return self._det_area[:self._last[0] * self.K].view(self._last[0], self.K)

    @property
    def truth_area(self):
        b, n = self._last
        return self._truth_area[:b * n].view(b, n)

    @property
    def det_truth(self):
        return self._det_truth[:self._last[0] * self.K * 2 * self.T].view(self._last[0], self.K, 2, self.T)

    def reset(self):
        self._state.zero_()
        self._images = 0

    def reserve(self, images):
        """Make room in the log for `images` images in all (a device-to-device copy of the log so far on the
        current stream; no synchronisation). Call it before capturing `update` in a graph."""
        images = int(images)
        if images <= self.capacity:
            return
        if self._fixed:
            raise ValueError(f"the log was built for {self.capacity} images")
        capacity = max(images, 2 * self.capacity)
        state = self._new_state(capacity)
        used = self._head + self.capacity * self.K * 4
        state[:used].copy_(self._state[:used], non_blocking=True)
        self._state, self.capacity = state, capacity

    def _grown(self, B, N):
        """An evaluator for at least B images and N truths per image that goes on with the same state."""
        other = DeviceYolactEvaluator(max(B, self.B), self.K, max(N, self.N), self.C, self.hw, self.device,
                                      self._host_thresholds)
        other._state, other.capacity = self._state, self.capacity
        other._images, other._fixed = self._images, self._fixed
        return other

    def _direct(self, t, dtypes, shape):
        return t.dtype in dtypes and t.device == self.device and t.is_contiguous() and tuple(t.shape) == shape

    def _truths(self, batch, valid, label, box):
        """(valid, label, box, n): the caller's tensors where the kernels can read them as they are (on the
        device, bool / uint8, int64, fp32, contiguous, exactly `batch` images, n >= 1), else the static
        buffers filled from them, with the images' missing truths invalid."""
        for name, t in (("valid", valid), ("label", label), ("box", box)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if valid.dim() != 2 or valid.shape[0] != batch:
            raise ValueError(f"valid must be [{batch}, n], got {list(valid.shape)}")
        n = valid.shape[1]
        if n > self.N:
            raise ValueError(f"{n} truths per image, the evaluator takes {self.N}")
        for name, t, shape in (("label", label, (batch, n)), ("box", box, (batch, n, 4))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        if n >= 1 and self._direct(valid, (torch.bool, torch.uint8), (batch, n)) \
                and self._direct(label, (torch.int64,), (batch, n)) \
                and self._direct(box, (torch.float32,), (batch, n, 4)):
            return valid, label, box, n
        self.valid.zero_()
        if n:
            self.valid[:batch, :n].copy_(valid.to(torch.bool), non_blocking=True)
            self.label[:batch, :n].copy_(label, non_blocking=True)
            self.box[:batch, :n].copy_(box, non_blocking=True)
        return self.valid, self.label, self.box, self.N

    def _device_tensor(self, t, name, dtypes, shape_tail, batch):
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
            raise ValueError(f"{name} must be a torch tensor of {' / '.join(str(d) for d in dtypes)}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the evaluator on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail) or t.shape[0] < batch:
            raise ValueError(f"{name} must be [>= {batch}, {', '.join(str(s) for s in shape_tail)}], got "
                             f"{list(t.shape)}")
        return t

    def update(self, bits, counts, confidence, records, seg, valid, label, box, batch=None):
        """Add one batch. On the device: bits [>= batch, K, H, ceil(W / 32)] uint32 (frame_masks'), counts
        [>= batch] int32, confidence [>= batch, K, C+1] and records [>= batch, K, 8] fp32 of one
        detection_records call (the detector's buffers as they are), seg [batch, H, W] uint8. The truths
        valid [batch, n] bool, label [batch, n] int64, box [batch, n, 4] (y, x, h, w) with n <= N are read
        as they are when they are device tensors of those types, else staged. `batch` (default: all the
        images of `bits`) may be smaller than B: the last batch of a loader. ValueError before any launch
        otherwise. Returns det_truth [batch, K, 2, T]."""
        if not isinstance(bits, torch.Tensor):
            raise ValueError(f"bits must be a torch tensor, got {type(bits).__name__}")
        batch = bits.shape[0] if batch is None else int(batch)
        if not 1 <= batch <= min(self.B, bits.shape[0]):
            raise ValueError(f"batch must be in 1..{min(self.B, bits.shape[0])} (the evaluator's B and the images of "
                             f"bits), got {batch}")
        H, W = self.hw
        K, C, T = self.K, self.C, self.T
        self._device_tensor(bits, "bits", (torch.uint32, torch.int32), (K, H, (W + 31) // 32), batch)
        self._device_tensor(counts, "counts", (torch.int32,), (), batch)
        self._device_tensor(confidence, "confidence", (torch.float32,), (K, C + 1), batch)
        self._device_tensor(records, "records", (torch.float32,), (K, 8), batch)
        self._device_tensor(seg, "seg", (torch.uint8,), (H, W), batch)
        if seg.shape[0] != batch:
            raise ValueError(f"seg must hold exactly {batch} images, got {seg.shape[0]}")
        v, l, bx, n = self._truths(batch, valid, label, box)
        if self._images + batch > self.capacity and not self._fixed:
            self.reserve(self._images + batch)
        self._images += batch
        self._last = (batch, n)
        lib, stream = _lib.lib(), _lib.stream_of(self.device)
        _lib.check(lib.tv_yolact_mask_overlap(_vp(bits), _vp(counts), _vp(seg), _vp(v), batch, K, n, H, W,
                                              _vp(self._inter), _vp(self._det_area), _vp(self._truth_area), stream),
                   "yolact_mask_overlap")
        state = self._state
        _lib.check(lib.tv_yolact_evaluate_match(
            _vp(confidence), _vp(records), _vp(counts), _vp(v), _vp(l), _vp(bx), _vp(self._inter), _vp(self._det_area),
            _vp(self._truth_area), _vp(self.iou_thresholds), batch, K, n, C, T, _vp(state),
            ctypes.c_void_p(state.data_ptr() + 4 * self._head), self.capacity, _vp(self._det_truth),
            ctypes.c_void_p(state.data_ptr() + 8), stream), "yolact_evaluate_match")
        return self.det_truth

    def host_state(self):
        """(cursor, totals [C+2] int64, log [capacity, K, 4] int32) on the host: ONE device-to-host copy,
        which waits for the launches so far."""
        host = self._state[:self._head + self.capacity * self.K * 4].cpu()
        return (int(host[:2].view(torch.int64)[0]), host[2:2 + 2 * (self.C + 2)].view(torch.int64).numpy(),
                host[self._head:].view(self.capacity, self.K, 4).numpy())

    def result(self) -> YolactEvaluation:
        """The data set's average precision (ONE device-to-host copy of the log, the totals and the
        cursor). ValueError if a valid truth had a label outside 1..C, if more images were logged than the
        log holds, or if a logged score is NaN; ZeroDivisionError without any truth."""
        cursor, totals, log = self.host_state()
        if int(totals[self.C + 1]) > 0:
            raise ValueError(f"{int(totals[self.C + 1])} valid truths carry a label outside 1..{self.C}")
        if cursor > self.capacity:
            raise ValueError(f"{cursor} images were logged, the log holds {self.capacity}: reserve() before replaying "
                             f"a captured graph")
        return average_precision(log[:cursor], totals[:self.C + 1], self.T, self._host_thresholds)


def _field(t, device, dtype=None):
    t = torch.as_tensor(t)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to(device, non_blocking=True).contiguous()


def evaluate_average_precision(model, data_loader, device, top_k=100, nms_iou_threshold=0.5, confidence_threshold=0.05,
                               iou_thresholds=None, max_batches=None) -> YolactEvaluation:
    """Box and mask average precision of `model` (a Yolact on the native backbone) over a loader of
    SegmentationSample batches after collate_samples (train.py:123-156), duck-typed: .img [B, 3, in_h,
    in_w] fp32 normalised, .seg [B, in_h, in_w] uint8, .valid [B, n] bool, .classifications [B, n] int64,
    .bounding_boxes [B, n, 4] (y, x, h, w). img_valid is not read: seg == 254 carries it. The fields are
    moved to `device` here. Per batch: the detector (top_k, nms_iou_threshold, confidence_threshold;
    frame_masks="bilinear" at the image size), one detection_records call for the softmax rows, update.
    Nothing reaches the host until the end (one copy). `max_batches`: stop after that many (None: all)."""
    from .yolact import YolactDetector, detection_records
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the evaluation runs on the GPU, got device {device}")
    detectors, evaluator = {}, None
    batches = data_loader if max_batches is None else islice(data_loader, int(max_batches))
    with torch.cuda.device(device), torch.no_grad():
        for sample in batches:
            img = _field(sample.img, device, torch.float32)
            seg = _field(sample.seg, device, torch.uint8)
            valid = _field(sample.valid, device, torch.bool)
            label = _field(sample.classifications, device, torch.int64)
            box = _field(sample.bounding_boxes, device, torch.float32)
            if img.dim() != 4 or img.shape[1] != 3:
                raise ValueError(f"img must be [B, 3, in_h, in_w], got {list(img.shape)}")
            B, hw = img.shape[0], (img.shape[2], img.shape[3])
            if (B, hw) not in detectors:
                det = YolactDetector(model, B, hw, int(top_k), img.device, frame_masks="bilinear")
                conf = torch.zeros((B, det.K, det.head_out[0].shape[2]), dtype=torch.float32, device=img.device)
                detectors[(B, hw)] = (det, conf)
            det, conf = detectors[(B, hw)]
            found = det(img, nms_iou_threshold, confidence_threshold)
            detection_records(det.head_out[0], det.box, det.det, det.counts, out=det.records, confidence_out=conf)
            N = max(int(valid.shape[1]), 1)
            if evaluator is None:
                evaluator = DeviceYolactEvaluator(B, det.K, N, conf.shape[2] - 1, hw, img.device, iou_thresholds)
            elif hw != evaluator.hw:
                raise ValueError(f"images of {hw} after images of {evaluator.hw}: one evaluation, one size")
            elif B > evaluator.B or N > evaluator.N:
                evaluator = evaluator._grown(B, N)
            evaluator.update(found.bits, found.counts, conf, det.records, seg, valid, label, box, batch=B)
        if evaluator is None:  # an empty loader: no truth
            raise ZeroDivisionError("division by zero")
        return evaluator.result()

