"""Training augmentation on the GPU: one sample of the reference's albumentations pipelines
(yolact/scripts/train.py:413-455, centernet/scripts/train.py:144-167) per frame, applied to u8 frames
in two launches (csrc/augment.hip; the contract is tv_augment_frames' in include/tauv_vision_amd.h).

The host samples one record per image (float64, a torch.Generator on the CPU: reproducible); the device
work is a pure function of (frames, seg, records, seed). Resize, flips, ShiftScaleRotate and Perspective
compose into ONE homography and one bilinear resampling; colour, noise, blur and Normalize follow in the
same kernel. albumentations and cv2 are not needed (and their pixel values are not reproduced: the
sampled distribution of transforms is the reference's, the arithmetic is DESIGN §20's).

In the reference's yolact train.py, replace `train_transform` and the loader's per-image call by
    params = sample_yolact_params(train_config, model_config, src_hw, B, generator)
    sample = augment_segmentation_batch(sample_u8, params, augmenter, seed)
and in the centernet train.py by sample_centernet_params / augment_pose_batch; the results go into
tauv_vision_amd.yolact_loss.loss and tauv_vision_amd.loss.loss as they are.

Departures from the reference's pipeline: one resampling instead of three; a fixed colour
order (albumentations' ColorJitter shuffles it); no rounding to u8 between the stages; the blur after the
warp; noise drawn per destination pixel; a hard frame edge (a destination pixel whose source position is
outside the frame is padding, no partial coverage); the contrast mean over the source frame; truth rows
are never compacted; no PiecewiseAffine.
"""
import ctypes
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from . import _lib
from .loss import PoseSample

REC = 32  # fp32 slots per record (csrc/augment.hip)
MINV, PERM, BRIGHTNESS, CONTRAST, SATURATION, HUE, SAT_SHIFT, VAL_SHIFT, NOISE_SIGMA, BLUR_K = \
    0, 9, 12, 13, 14, 15, 16, 17, 18, 19
MASK_VALUE = 254  # the reference's mask_value / mask_pad_val: img_valid = seg != 254
BLUR_KS = (1, 3, 5, 7)
_F64 = torch.float64


@dataclass
class AugmentParams:
    """One sampled transform per frame: `records` [B, 32] fp32 as the kernel reads them (host tensor) and
    the forward matrices `matrices` [B, 3, 3] float64 (source to destination continuous pixel coordinates),
    which the truth goes through. `min_visibility` is carried for transform_boxes."""
    records: torch.Tensor
    matrices: torch.Tensor
    src_hw: Tuple[int, int]
    dst_hw: Tuple[int, int]
    min_visibility: float = 0.0

    @property
    def B(self):
        return self.records.shape[0]


def _hw(hw, name):
    h, w = int(hw[0]), int(hw[1])
    if h < 1 or w < 1:
        raise ValueError(f"{name} must be two positive sizes, got {tuple(hw)}")
    return h, w


def resize_matrix(src_hw, dst_hw):
    """S = diag(Wd / Ws, Hd / Hs, 1), float64."""
    (hs, ws), (hd, wd) = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
    return torch.diag(torch.tensor([wd / ws, hd / hs, 1.0], dtype=_F64))


def flip_matrix(dst_hw, horizontal, vertical):
    """F: x -> Wd - x and / or y -> Hd - y in continuous destination coordinates."""
    hd, wd = _hw(dst_hw, "dst_hw")
    m = torch.eye(3, dtype=_F64)
    if horizontal:
        m[0, 0], m[0, 2] = -1.0, float(wd)
    if vertical:
        m[1, 1], m[1, 2] = -1.0, float(hd)
    return m


def shift_scale_rotate_matrix(dst_hw, shift_xy=(0.0, 0.0), scale=1.0, angle_deg=0.0):
    """R: rotate by angle_deg (counter-clockwise on the screen, as cv2.getRotationMatrix2D) and scale
    about the destination centre, then shift by fractions (of Wd, of Hd) — albumentations' ShiftScaleRotate."""
    hd, wd = _hw(dst_hw, "dst_hw")
    cx, cy = wd / 2.0, hd / 2.0
    a = math.radians(float(angle_deg))
    c, s = math.cos(a) * float(scale), math.sin(a) * float(scale)
    dx, dy = float(shift_xy[0]) * wd, float(shift_xy[1]) * hd
    return torch.tensor([[c, s, (1 - c) * cx - s * cy + dx],
                         [-s, c, s * cx + (1 - c) * cy + dy],
                         [0.0, 0.0, 1.0]], dtype=_F64)


def homography_from_points(src_xy, dst_xy):
    """The 3 x 3 matrix (last entry 1) that maps four points to four points, float64."""
    src = torch.as_tensor(src_xy, dtype=_F64).reshape(4, 2)
    dst = torch.as_tensor(dst_xy, dtype=_F64).reshape(4, 2)
    A = torch.zeros((8, 8), dtype=_F64)
    rhs = torch.zeros(8, dtype=_F64)
    for i in range(4):
        x, y = src[i]
        u, v = dst[i]
        A[2 * i] = torch.tensor([x, y, 1, 0, 0, 0, -u * x, -u * y], dtype=_F64)
        A[2 * i + 1] = torch.tensor([0, 0, 0, x, y, 1, -v * x, -v * y], dtype=_F64)
        rhs[2 * i], rhs[2 * i + 1] = u, v
    h = torch.linalg.solve(A, rhs)
    return torch.cat([h, torch.ones(1, dtype=_F64)]).reshape(3, 3)


def perspective_matrix(dst_hw, corner_offsets):
    """P of albumentations' Perspective(scale, keep_size=True, fit_output=False), restated from its
    documentation — PARITY UNPINNED (albumentations is not installed here and no fixture of it exists):
    four corner points are drawn at normally distributed distances (standard deviation `scale`, as a
    fraction of the frame, folded into [0, 0.32) by |.| mod 0.32) inward from the frame's corners; the
    quadrilateral they span is mapped onto the whole frame, which keep_size leaves at its size.
    corner_offsets [4, 2]: the (x, y) fractions for the top-left, top-right, bottom-right and bottom-left
    corner, each measured inward."""
    hd, wd = _hw(dst_hw, "dst_hw")
    o = torch.as_tensor(corner_offsets, dtype=_F64).reshape(4, 2)
    quad = torch.stack([torch.stack([o[0, 0], o[0, 1]]), torch.stack([1 - o[1, 0], o[1, 1]]),
                        torch.stack([1 - o[2, 0], 1 - o[2, 1]]), torch.stack([o[3, 0], 1 - o[3, 1]])])
    quad = quad * torch.tensor([wd, hd], dtype=_F64)
    full = torch.tensor([[0, 0], [wd, 0], [wd, hd], [0, hd]], dtype=_F64)
    return homography_from_points(quad, full)


def _per_frame(value, B, name, width=None):
    t = torch.as_tensor(value, dtype=_F64)
    shape = (B,) if width is None else (B, width)
    if t.dim() == len(shape) - 1:
        t = t.expand(shape)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be a scalar or {list(shape)}, got {list(t.shape)}")
    return t


def params_from_matrices(M, src_hw, dst_hw, perm=(0, 1, 2), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0,
                         sat_shift=0.0, val_shift=0.0, noise_sigma=0.0, blur_k=1, min_visibility=0.0) -> AugmentParams:
    """Records for the caller's own forward matrices M [B, 3, 3] (source to destination continuous pixel
    coordinates). Every other field is a scalar for all frames or one value per frame. ValueError for a
    singular matrix, a perm that is no permutation of (0, 1, 2), a blur_k outside {1, 3, 5, 7} or a
    negative noise_sigma."""
    src_hw, dst_hw = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
    M = torch.as_tensor(M, dtype=_F64)
    if M.dim() != 3 or tuple(M.shape[1:]) != (3, 3) or M.shape[0] < 1:
        raise ValueError(f"M must be [B, 3, 3], got {list(M.shape)}")
    B = M.shape[0]
    det = torch.linalg.det(M)
    if not bool(torch.isfinite(M).all()) or bool((det.abs() < 1e-12).any()):
        raise ValueError("M must be finite and invertible")
    minv = torch.linalg.inv(M)
    # a homography is defined up to a positive factor (the sign carries `w > 0`): keep m8 at 1 where it is
    # not tiny, so that the fp32 slots stay near the pixel scale
    m8 = minv[:, 2, 2].abs()
    minv = minv / torch.where(m8 > 1e-6, m8, torch.ones_like(m8)).view(B, 1, 1)
    # an affine M (flips, quarter turns, resizes) inverts in closed form: integer matrices stay exact
    affine = (M[:, 2, 0] == 0) & (M[:, 2, 1] == 0) & (M[:, 2, 2] == 1)
    a, b_, c, d_ = M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1]
    dd = a * d_ - b_ * c
    dd = torch.where(affine, dd, torch.ones_like(dd))
    ia, ib, ic, id_ = d_ / dd, -b_ / dd, -c / dd, a / dd
    tx, ty = M[:, 0, 2], M[:, 1, 2]
    zero, one = torch.zeros_like(a), torch.ones_like(a)
    closed = torch.stack([ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty), zero, zero, one], 1).view(B, 3, 3)
    minv = torch.where(affine.view(B, 1, 1), closed, minv)
    rec = torch.zeros((B, REC), dtype=_F64)
    rec[:, MINV:MINV + 9] = minv.reshape(B, 9)
    p = _per_frame(perm, B, "perm", 3)
    if not bool((p.sort(dim=1).values == torch.tensor([0.0, 1.0, 2.0], dtype=_F64)).all()):
        raise ValueError("perm must be a permutation of (0, 1, 2)")
    rec[:, PERM:PERM + 3] = p
    for slot, value, name in ((BRIGHTNESS, brightness, "brightness"), (CONTRAST, contrast, "contrast"),
                              (SATURATION, saturation, "saturation"), (HUE, hue, "hue"),
                              (SAT_SHIFT, sat_shift, "sat_shift"), (VAL_SHIFT, val_shift, "val_shift"),
                              (NOISE_SIGMA, noise_sigma, "noise_sigma"), (BLUR_K, blur_k, "blur_k")):
        rec[:, slot] = _per_frame(value, B, name)
    if not bool(torch.isfinite(rec).all()):
        raise ValueError("the record fields must be finite")
    if bool((rec[:, NOISE_SIGMA] < 0).any()):
        raise ValueError("noise_sigma must be >= 0")
    if not all(float(k) in BLUR_KS for k in rec[:, BLUR_K]):
        raise ValueError(f"blur_k must be one of {BLUR_KS}")
    return AugmentParams(rec.to(torch.float32), M.clone(), src_hw, dst_hw, float(min_visibility))


def identity_params(B, src_hw, dst_hw) -> AugmentParams:
    """The identity record for every frame: a pure resize (nothing at all at equal sizes)."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    return params_from_matrices(resize_matrix(src_hw, dst_hw).expand(B, 3, 3), src_hw, dst_hw)


class _Draw:
    """float64 draws from one CPU generator, in call order."""

    def __init__(self, generator):
        self.g = generator

    def uniform(self, lo, hi):
        return float(lo) + (float(hi) - float(lo)) * float(torch.rand((), generator=self.g, dtype=_F64))

    def happens(self, p):
        return float(torch.rand((), generator=self.g, dtype=_F64)) < float(p)

    def normal(self, n):
        return torch.randn(n, generator=self.g, dtype=_F64)

    def integer(self, lo, hi):
        """uniform integer in [lo, hi]"""
        return int(torch.randint(int(lo), int(hi) + 1, (), generator=self.g))

    def permutation(self, n):
        return torch.randperm(n, generator=self.g)


def _pair(v):
    try:
        lo, hi = v
    except TypeError:
        lo, hi = -abs(v), abs(v)
    return float(lo), float(hi)


def _odd_kernel(d, limit):
    lo, hi = (3, int(limit)) if isinstance(limit, (int, float)) else (int(limit[0]), int(limit[1]))
    lo, hi = max(lo | 1, 1), hi if hi % 2 else hi - 1
    if lo > hi or hi > BLUR_KS[-1]:
        raise ValueError(f"blur_limit must give odd kernels within 1..{BLUR_KS[-1]}, got {limit}")
    return lo + 2 * d.integer(0, (hi - lo) // 2)


def _perspective_offsets(d, limits):
    lo, hi = _pair(limits) if not isinstance(limits, (int, float)) else (0.0, float(limits))
    scale = d.uniform(lo, hi)
    return torch.remainder((d.normal(8) * scale).abs(), 0.32).reshape(4, 2)


def sample_yolact_params(train_config, model_config, src_hw, B, generator) -> AugmentParams:
    """One record per frame from the reference's TrainConfig (yolact/model/config.py:52-92, duck-typed) as
    train.py:413-455 uses it; destination = (model_config.in_h, model_config.in_w). Per frame, in this
    order, each draw taken only when its `*_p` fires: channel_shuffle_p (a random permutation);
    color_jitter_p (brightness, contrast, saturation uniform in [max(0, 1 - a), 1 + a], hue uniform in
    [-h, h]); gaussian_noise_p (variance uniform in gaussian_noise_var_limit, sigma = sqrt(var));
    horizontal_flip_p; vertical_flip_p; blur_p (an odd kernel uniform in blur_limit); ssr_p (shift x and y
    uniform in ssr_shift_limit, scale 1 + uniform in ssr_scale_limit, angle uniform in ssr_rotate_limit
    degrees); perspective_p (perspective_matrix with scale uniform in perspective_scale_limit).
    M = P R F S. min_visibility is carried for the truth. The same generator state gives the same records."""
    tc, d = train_config, _Draw(generator)
    src_hw, dst_hw = _hw(src_hw, "src_hw"), _hw((model_config.in_h, model_config.in_w), "model_config.in_h/in_w")
    S = resize_matrix(src_hw, dst_hw)
    fields = {k: [] for k in ("perm", "brightness", "contrast", "saturation", "hue", "noise_sigma", "blur_k")}
    Ms = []
    for _ in range(int(B)):
        perm = d.permutation(3).tolist() if d.happens(tc.channel_shuffle_p) else [0, 1, 2]
        br = ct = sat = 1.0
        hue = 0.0
        if d.happens(tc.color_jitter_p):
            br = d.uniform(max(0.0, 1 - tc.color_jitter_brightness), 1 + tc.color_jitter_brightness)
            ct = d.uniform(max(0.0, 1 - tc.color_jitter_contrast), 1 + tc.color_jitter_contrast)
            sat = d.uniform(max(0.0, 1 - tc.color_jitter_saturation), 1 + tc.color_jitter_saturation)
            hue = d.uniform(-tc.color_jitter_hue, tc.color_jitter_hue)
        sigma = math.sqrt(d.uniform(*_pair(tc.gaussian_noise_var_limit))) if d.happens(tc.gaussian_noise_p) else 0.0
        hflip, vflip = d.happens(tc.horizontal_flip_p), d.happens(tc.vertical_flip_p)
        k = _odd_kernel(d, tc.blur_limit) if d.happens(tc.blur_p) else 1
        R = torch.eye(3, dtype=_F64)
        if d.happens(tc.ssr_p):
            shift = (d.uniform(*_pair(tc.ssr_shift_limit)), d.uniform(*_pair(tc.ssr_shift_limit)))
            scale = 1.0 + d.uniform(*_pair(tc.ssr_scale_limit))
            R = shift_scale_rotate_matrix(dst_hw, shift, scale, d.uniform(*_pair(tc.ssr_rotate_limit)))
        P = torch.eye(3, dtype=_F64)
        if d.happens(tc.perspective_p):
            P = perspective_matrix(dst_hw, _perspective_offsets(d, tc.perspective_scale_limit))
        Ms.append(P @ R @ flip_matrix(dst_hw, hflip, vflip) @ S)
        for name, v in (("perm", perm), ("brightness", br), ("contrast", ct), ("saturation", sat), ("hue", hue),
                        ("noise_sigma", sigma), ("blur_k", k)):
            fields[name].append(v)
    return params_from_matrices(torch.stack(Ms), src_hw, dst_hw, min_visibility=float(tc.min_visibility), **fields)


CENTERNET_DEFAULTS = dict(
    crop_p=0.25, crop_min_max_height=(260 / 360, 1.0), crop_w2h_ratio=640 / 360,   # train.py:146-152
    hsv_p=0.5, hue_shift_limit=(-20, 20), sat_shift_limit=(-30, 30), val_shift_limit=(-20, 20),  # :153-158
    flip_p=0.5,                                      # A.Flip(): p = 0.5, one of horizontal, vertical, both
    blur_p=0.5, blur_limit=(3, 7),                   # A.Blur(): blur_limit = 7 -> (3, 7), p = 0.5
    noise_p=0.5, noise_var_limit=(10.0, 50.0),       # A.GaussNoise(): var_limit = (10, 50), mean = 0, p = 0.5
    min_visibility=0.0)                              # A.BboxParams default


def sample_centernet_params(src_hw, dst_hw, B, generator, **overrides) -> AugmentParams:
    """One record per frame from the literals of the reference's centernet train.py:146-161 and, where it
    passes none, albumentations 1.3's defaults — each default PARITY UNPINNED (albumentations is not
    installed here; restated from its documentation):
      RandomSizedCrop(min_max_height=(260, 360), w2h_ratio=640 / 360, p=0.25): a window of height uniform
        in that range (kept as a fraction of a 360-row frame), width = height * w2h_ratio (at most the
        frame), anywhere in the frame, resized to the destination — here S, the crop window mapped to the
        full frame;
      HueSaturationValue((-20, 20), (-30, 30), (-20, 20), p=0.5): hue = shift / 180, sat_shift = shift / 255,
        val_shift = shift / 255 (cv2's 8-bit HSV ranges);
      Flip(): p = 0.5, then horizontal, vertical or both with equal chance (d in {1, 0, -1});
      Blur(): blur_limit = 7, i.e. an odd kernel in (3, 7), p = 0.5;
      GaussNoise(): var_limit = (10, 50), mean = 0, p = 0.5 (per channel noise).
    PiecewiseAffine(scale=[0.01, 0.02], nb_rows=4, nb_cols=4, p=0.1) is NOT built: no frame takes it.
    `overrides` replace entries of CENTERNET_DEFAULTS."""
    unknown = set(overrides) - set(CENTERNET_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown overrides {sorted(unknown)}; known: {sorted(CENTERNET_DEFAULTS)}")
    c = SimpleNamespace(**{**CENTERNET_DEFAULTS, **overrides})
    d = _Draw(generator)
    (hs, ws), dst_hw = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
    hd, wd = dst_hw
    fields = {k: [] for k in ("hue", "sat_shift", "val_shift", "noise_sigma", "blur_k")}
    Ms = []
    for _ in range(int(B)):
        S = resize_matrix((hs, ws), dst_hw)
        if d.happens(c.crop_p):
            ch = d.uniform(*c.crop_min_max_height) * hs
            cw = min(ch * c.crop_w2h_ratio, float(ws))
            x0, y0 = d.uniform(0.0, ws - cw), d.uniform(0.0, hs - ch)
            S = torch.tensor([[wd / cw, 0, -x0 * wd / cw], [0, hd / ch, -y0 * hd / ch], [0, 0, 1]], dtype=_F64)
        hue = sat = val = 0.0
        if d.happens(c.hsv_p):
            hue = d.uniform(*_pair(c.hue_shift_limit)) / 180.0
            sat = d.uniform(*_pair(c.sat_shift_limit)) / 255.0
            val = d.uniform(*_pair(c.val_shift_limit)) / 255.0
        hflip = vflip = False
        if d.happens(c.flip_p):
            hflip, vflip = ((True, False), (False, True), (True, True))[d.integer(0, 2)]
        k = _odd_kernel(d, c.blur_limit) if d.happens(c.blur_p) else 1
        sigma = math.sqrt(d.uniform(*_pair(c.noise_var_limit))) if d.happens(c.noise_p) else 0.0
        Ms.append(flip_matrix(dst_hw, hflip, vflip) @ S)
        for name, v in (("hue", hue), ("sat_shift", sat), ("val_shift", val), ("noise_sigma", sigma), ("blur_k", k)):
            fields[name].append(v)
    return params_from_matrices(torch.stack(Ms), (hs, ws), dst_hw, min_visibility=float(c.min_visibility), **fields)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _require(t, name, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the augmenter on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


class DeviceAugmenter:
    """Static-buffer augmentation of B frames of src_hw to dst_hw: `__call__` copies the records to the
    device (one host-to-device copy from a pinned buffer) and runs the two launches on the current stream,
    with no allocation and no host synchronisation. `img` [B, 3, Hd, Wd] fp32 and `seg_out` [B, Hd, Wd]
    uint8 are the outputs, overwritten by every call. The pinned buffer is one: `load` first waits (on the
    host) for the copy the previous `load` queued, so a loop that never synchronises cannot overwrite
    records that an earlier call's kernels have yet to read; that wait ends when the previous copy has
    run, not when its kernels have. Graph capture: `load(params)` before the capture, then capture
    `augmenter(frames, seg, None, seed)` (a `load` inside a capture is refused: it would have to wait);
    a replay reads the frames' buffers, the device records as a later `load` left them, and the
    captured seed."""

    def __init__(self, B, src_hw, dst_hw, mean, std, device):
        B = int(B)
        if B < 1:
            raise ValueError(f"B must be >= 1, got {B}")
        self.src_hw, self.dst_hw = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
            raise ValueError(f"mean and std must be three values each with std non-zero, got {mean}, {std}")
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceAugmenter needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.B = B
        self._mean, self._std = (_lib.c_f32 * 3)(*mean), (_lib.c_f32 * 3)(*std)
        need = _lib.c_i64(0)
        _lib.check(_lib.lib().tv_augment_workspace_size(B, self.src_hw[0], self.src_hw[1], ctypes.byref(need)),
                   "augment_workspace_size")
        self._ws_bytes = int(need.value)
        self.workspace = torch.empty(self._ws_bytes // 8, dtype=torch.float64, device=dev)
        self.records = torch.zeros((B, REC), dtype=torch.float32, device=dev)
        self._host_records = torch.zeros((B, REC), dtype=torch.float32).pin_memory()
        self.img = torch.empty((B, 3) + self.dst_hw, dtype=torch.float32, device=dev)
        self.seg_out = torch.empty((B,) + self.dst_hw, dtype=torch.uint8, device=dev)
        self._copied = torch.cuda.Event()  # recorded after every records copy: guards the pinned buffer
        self._loaded = False

    def load(self, params: AugmentParams):
        """Check the records on the host and copy them to the device (asynchronously, on the current stream)."""
        if not isinstance(params, AugmentParams):
            raise ValueError(f"params must be AugmentParams, got {type(params).__name__}")
        rec = params.records
        if tuple(rec.shape) != (self.B, REC) or rec.dtype != torch.float32 or rec.is_cuda:
            raise ValueError(f"params.records must be a host fp32 [{self.B}, {REC}] tensor, got {rec.dtype} "
                             f"{list(rec.shape)} on {rec.device}")
        if tuple(params.src_hw) != self.src_hw or tuple(params.dst_hw) != self.dst_hw:
            raise ValueError(f"params are for {params.src_hw} -> {params.dst_hw}, the augmenter for {self.src_hw} -> "
                             f"{self.dst_hw}")
        k = rec[:, BLUR_K]
        if not all(float(v) in BLUR_KS for v in k):
            raise ValueError(f"blur_k must be one of {BLUR_KS}")
        if float(k.max()) > min(self.dst_hw):
            raise ValueError(f"blur_k = {int(k.max())} exceeds the destination's smaller side {min(self.dst_hw)} "
                             "(reflect padding reaches one image size at the most)")
        if not bool(torch.isfinite(rec).all()):
            raise ValueError("params.records must be finite")
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("load(params) inside a graph capture: load before the capture and call with params=None")
        # the previous load's copy may still be queued behind GPU work and reads the pinned buffer when it
        # runs: wait for it before writing the buffer again
        if self._loaded:
            self._copied.synchronize()
        self._host_records.copy_(rec)
        self.records.copy_(self._host_records, non_blocking=True)
        self._copied.record(torch.cuda.current_stream(self.device))
        self._loaded = True

    def __call__(self, frames_u8, seg_u8, params, seed):
        """frames_u8 [B, Hs, Ws, 3] uint8 and seg_u8 [B, Hs, Ws] uint8 (or None) on the device, contiguous;
        params: AugmentParams, or None to run on the records of the last `load`; seed: the noise key
        (0 .. 2^64 - 1). -> (img, seg_out) — the augmenter's buffers; seg_out is None without seg_u8.
        ValueError before any launch for anything else."""
        _require(frames_u8, "frames_u8", torch.uint8, self.device)
        if tuple(frames_u8.shape) != (self.B,) + self.src_hw + (3,):
            raise ValueError(f"frames_u8 must be {[self.B, *self.src_hw, 3]}, got {list(frames_u8.shape)}")
        if seg_u8 is not None:
            _require(seg_u8, "seg_u8", torch.uint8, self.device)
            if tuple(seg_u8.shape) != (self.B,) + self.src_hw:
                raise ValueError(f"seg_u8 must be {[self.B, *self.src_hw]}, got {list(seg_u8.shape)}")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be in 0 .. 2^64 - 1, got {seed}")
        if params is not None:
            self.load(params)
        elif not self._loaded:
            raise ValueError("no records on the device: pass params or call load(params) first")
        seg_out = self.seg_out if seg_u8 is not None else None
        _lib.check(_lib.lib().tv_augment_frames(
            _vp(frames_u8), _vp(seg_u8), self.B, self.src_hw[0], self.src_hw[1], self.dst_hw[0], self.dst_hw[1],
            _vp(self.records), ctypes.c_uint64(seed), self._mean, self._std, _vp(self.img), _vp(seg_out),
            _vp(self.workspace), self._ws_bytes, _lib.stream_of(self.device)), "augment_frames")
        return self.img, seg_out


def _project(M, x, y):
    """(x', y', w) of points x, y [B, N] through M [B, 3, 3], float64."""
    m = M.view(M.shape[0], 1, 9)
    w = m[..., 6] * x + m[..., 7] * y + m[..., 8]
    return (m[..., 0] * x + m[..., 1] * y + m[..., 2]) / w, (m[..., 3] * x + m[..., 4] * y + m[..., 5]) / w, w


def _truth_args(t, valid, params, width, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != width or t.shape[0] != params.B:
        raise ValueError(f"{name} must be [{params.B}, N, {width}], got "
                         f"{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if not isinstance(valid, torch.Tensor) or tuple(valid.shape) != tuple(t.shape[:2]):
        raise ValueError(f"valid must be {list(t.shape[:2])}")
    return t.to(_F64), valid.to(torch.bool), params.matrices.to(t.device)


def transform_boxes(box_yxhw, valid, params: AugmentParams, min_visibility=None):
    """Boxes (y, x, h, w), normalised to the source frame, through the frames' matrices: the four corners
    go through M to an enclosing axis-aligned box, clipped to [0, 1] and normalised to the destination.
    -> (box [B, N, 4] in the input's dtype, valid [B, N] bool): valid stays true iff the clipped area is
    > 0 and clipped / unclipped area > min_visibility (default: params.min_visibility); a corner behind
    the homography's horizon drops the box. Rows are NEVER compacted — a dropped truth turns invalid in
    place (its box is zero), because the YOLACT seg map stores the truth's row index. Pure torch, float64
    inside, on the tensors' device."""
    b, v, M = _truth_args(box_yxhw, valid, params, 4, "box_yxhw")
    mv = params.min_visibility if min_visibility is None else float(min_visibility)
    (hs, ws), (hd, wd) = params.src_hw, params.dst_hw
    cy, cx, h, w = b.unbind(-1)
    xs = torch.stack([cx - w / 2, cx + w / 2, cx + w / 2, cx - w / 2], -1) * ws
    ys = torch.stack([cy - h / 2, cy - h / 2, cy + h / 2, cy + h / 2], -1) * hs
    B, N = v.shape
    px, py, pw = _project(M, xs.reshape(B, N * 4), ys.reshape(B, N * 4))
    px, py, pw = (px / wd).view(B, N, 4), (py / hd).view(B, N, 4), pw.view(B, N, 4)
    x0, x1, y0, y1 = px.amin(-1), px.amax(-1), py.amin(-1), py.amax(-1)
    full = (x1 - x0) * (y1 - y0)
    cx0, cx1, cy0, cy1 = x0.clamp(0, 1), x1.clamp(0, 1), y0.clamp(0, 1), y1.clamp(0, 1)
    area = (cx1 - cx0) * (cy1 - cy0)
    ok = v & (pw > 0).all(-1) & torch.isfinite(full) & (area > 0) & (area > mv * full)
    out = torch.stack([(cy0 + cy1) / 2, (cx0 + cx1) / 2, cy1 - cy0, cx1 - cx0], -1)
    out = torch.where(ok.unsqueeze(-1), out, torch.zeros_like(out))
    return out.to(box_yxhw.dtype), ok


def transform_points(point_yx, valid, params: AugmentParams):
    """Points (y, x), normalised to the source frame, through the frames' matrices, normalised to the
    destination. -> (point [B, N, 2], valid [B, N] bool): valid stays true iff the image of the point lies
    in the frame (0 <= . < 1 on both axes, in front of the horizon). Rows are never compacted; a dropped
    point is zero. Pure torch, float64 inside."""
    p, v, M = _truth_args(point_yx, valid, params, 2, "point_yx")
    (hs, ws), (hd, wd) = params.src_hw, params.dst_hw
    px, py, pw = _project(M, p[..., 1] * ws, p[..., 0] * hs)
    px, py = px / wd, py / hd
    ok = v & (pw > 0) & (px >= 0) & (px < 1) & (py >= 0) & (py < 1)
    out = torch.stack([py, px], -1)
    out = torch.where(ok.unsqueeze(-1), out, torch.zeros_like(out))
    return out.to(point_yx.dtype), ok


@dataclass
class SegmentationSample:
    """The fields of the reference's collated SegmentationSample (datasets/load/segmentation_dataset.py)."""
    img: torch.Tensor              # [B, 3, in_h, in_w] fp32, normalised
    seg: torch.Tensor              # [B, in_h, in_w] uint8: the truth's row index, 254 = invalid image
    valid: torch.Tensor            # [B, N] bool
    classifications: torch.Tensor  # [B, N] int
    bounding_boxes: torch.Tensor   # [B, N, 4] (y, x, h, w) normalised
    img_valid: torch.Tensor        # [B, in_h, in_w] bool

    def truth(self):
        """The truth tuple of tauv_vision_amd.yolact_loss.loss."""
        return self.valid, self.classifications, self.bounding_boxes, self.seg, self.img_valid


def augment_segmentation_batch(sample_u8, params: AugmentParams, augmenter: DeviceAugmenter, seed) -> SegmentationSample:
    """A collated batch with `img` as u8 frames [B, Hs, Ws, 3] and `seg` [B, Hs, Ws] uint8 (on the host or
    the device) -> the augmented SegmentationSample on the augmenter's device. `img` and `seg` are the
    augmenter's buffers (clone to keep them past the next call); img_valid = seg != 254; the boxes go
    through transform_boxes, their rows in place."""
    dev = augmenter.device
    frames = sample_u8.img.to(dev).contiguous()
    seg = sample_u8.seg.to(device=dev, dtype=torch.uint8).contiguous()
    img, seg_out = augmenter(frames, seg, params, seed)
    box, valid = transform_boxes(sample_u8.bounding_boxes.to(dev), sample_u8.valid.to(dev), params)
    return SegmentationSample(img, seg_out, valid, sample_u8.classifications.to(dev), box, seg_out != MASK_VALUE)


def augment_pose_batch(sample_u8, params: AugmentParams, augmenter: DeviceAugmenter, seed) -> PoseSample:
    """A collated PoseSample with `img` as u8 frames [B, Hs, Ws, 3] -> tauv_vision_amd.loss.PoseSample on
    the augmenter's device: centre and size from transform_boxes of (center, size), keypoints through
    transform_points (a keypoint also drops with its object); label, angles and depth are carried
    unchanged, as the reference carries them. Rows stay in place."""
    dev = augmenter.device
    img, _ = augmenter(sample_u8.img.to(dev).contiguous(), None, params, seed)

    def on(name):
        t = getattr(sample_u8, name, None)
        return None if t is None else t.to(dev)

    size = on("size")
    center = on("center")
    box = torch.cat([center, size if size is not None else torch.zeros_like(center)], -1)
    if size is None:  # centres alone: a point's rule
        center, valid = transform_points(center, on("valid"), params)
    else:
        box, valid = transform_boxes(box, on("valid"), params)
        center, size = box[..., :2].contiguous(), box[..., 2:].contiguous()
    kv, kc, ko = on("keypoint_valid"), on("keypoint_center"), on("keypoint_object_index")
    if kc is not None and kv is not None:
        kc, kv = transform_points(kc, kv, params)
        if ko is not None and valid.shape[1] > 0:
            kv = kv & torch.gather(valid, 1, ko.long().clamp(0, valid.shape[1] - 1))
    return PoseSample(valid=valid, label=on("label"), center=center, keypoint_valid=kv, keypoint_label=on("keypoint_label"),
                      keypoint_center=kc, keypoint_object_index=ko, img=img, size=size, roll=on("roll"),
                      pitch=on("pitch"), yaw=on("yaw"), depth=on("depth"))
