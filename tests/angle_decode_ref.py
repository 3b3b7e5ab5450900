"""Test infrastructure of the orientation decode (tv_decode_angles, csrc/decode.hip): the reference's
angle_decode (decode.py:291-316) restated in torch at a chosen precision, the encoder that restates the
targets angle_loss trains against (loss.py:334-376), the input recipe of the device tests and their
comparison.

The restatement in fp32 is bit-exact to the reference on the CPU (tests/golden/angles_*.npz,
test_angle_decode_ref_cpu.py); the same lines in float64 are the yardstick of the device tests.

The inputs' condition. Which bin is decoded hangs on `s1 > s0` between two fp32 softmax scores. Where the
scores nearly tie, an fp32 `expf` that differs by one ulp from torch's flips the choice and the decoded
angle jumps by about pi — a difference of libm, not an error. `conditioned_bins` therefore draws the
logits with |b1-b0| <= 8, |b3-b2| <= 8 and |(b1-b0) - (b3-b2)| >= 0.5: with s = sigmoid(difference),
ds/dx = s(1-s) >= sigmoid(8)(1-sigmoid(8)) = 3.35e-4 on [-8, 8], so the scores differ by at least
0.5 * 3.35e-4 = 1.7e-4, three orders above an fp32 ulp at 1. `assert_conditioned` checks it on the very
fp32 inputs a test uses; no cell is then left out of a comparison.
"""
from math import pi

import numpy as np
import torch

MAX_DIFF, MIN_GAP = 8.0, 0.5
FLOOR = 2.0 ** -20  # the project's floor on an fp32 bar


def angle_decode_ref(predicted_bin, predicted_offset, theta_range, dtype=torch.float32):
    """angle_decode on [..., 4] bins / offsets (numpy or torch) in `dtype`; theta_range a Python float or
    an array broadcastable to the leading shape (a per-cell period: NaN gives NaN). numpy out."""
    b = torch.as_tensor(np.asarray(predicted_bin)).to(dtype)
    o = torch.as_tensor(np.asarray(predicted_offset)).to(dtype)
    s0 = torch.softmax(b[..., 0:2], dim=-1)[..., 1]
    s1 = torch.softmax(b[..., 2:4], dim=-1)[..., 1]
    a0 = pi / 2 + torch.atan2(o[..., 0], o[..., 1])
    a1 = -pi / 2 + torch.atan2(o[..., 2], o[..., 3])
    ang = torch.where(s1 > s0, a1, a0) % (2 * pi)
    if isinstance(theta_range, (int, float)):
        return (ang * (theta_range / (2 * pi))).numpy()
    scale = torch.as_tensor(np.asarray(theta_range, dtype=np.float64) / (2 * pi)).to(dtype)
    return (ang * scale).numpy()


def angle_in_range(angles, lo, hi):
    """loss.py:320-331 on float64 numpy."""
    lo, hi, angles = lo % (2 * pi), hi % (2 * pi), angles % (2 * pi)
    return ((lo <= angles) & (angles <= hi)) if lo < hi else ((lo <= angles) | (angles <= hi))


def angle_encode(theta, modulo, bin_overlap, logit=10.0):
    """What angle_loss trains the heads towards for truth angles `theta` (float64 numpy [n]) of period
    `modulo`: bins [n, 4] fp32 with +-logit on [outside, inside] of each bin, offsets [n, 4] fp32 with
    (sin, cos) of the stretched angle about each bin's centre."""
    t = (np.asarray(theta, np.float64) % modulo) * (2 * pi / modulo)
    bins = (pi / 2, -bin_overlap / 2, pi + bin_overlap / 2), (-pi / 2, -pi - bin_overlap / 2, bin_overlap / 2)
    b, o = [], []
    for c, lo, hi in bins:
        inside = angle_in_range(t, lo, hi)
        b += [np.where(inside, -logit, logit), np.where(inside, logit, -logit)]
        o += [np.sin(t - c), np.cos(t - c)]
    return np.stack(b, -1).astype(np.float32), np.stack(o, -1).astype(np.float32)


def circular_distance(a, b, period):
    """|a - b| on the circle of circumference `period` (float64)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % period
    return np.minimum(d, period - d)


def conditioned_bins(rng, shape):
    """fp32 bin logits [*shape, 4] under the module text's condition (margins for the fp32 rounding of
    b0 + difference: differences within 7.9, gaps of at least 0.51)."""
    d0 = rng.uniform(-7.9, 7.9, shape)
    d1 = rng.uniform(-7.9, 7.9, shape)
    bad = np.abs(d0 - d1) < 0.51
    while bad.any():
        d1[bad] = rng.uniform(-7.9, 7.9, int(bad.sum()))
        bad = np.abs(d0 - d1) < 0.51
    b0, b2 = rng.uniform(-3, 3, shape), rng.uniform(-3, 3, shape)
    return np.stack([b0, b0 + d0, b2, b2 + d1], -1).astype(np.float32)


def assert_conditioned(bins):
    b = np.asarray(bins, np.float64)
    d0, d1 = b[..., 1] - b[..., 0], b[..., 3] - b[..., 2]
    assert (np.abs(d0) <= MAX_DIFF).all() and (np.abs(d1) <= MAX_DIFF).all() and (np.abs(d0 - d1) >= MIN_GAP).all()
    s = lambda x: 1.0 / (1.0 + np.exp(-x))
    assert (np.abs(s(d0) - s(d1)) >= 1.7e-4).all()


def expected_angles(records, counts, heads, theta_range, H, W):
    """The angles [B, K, 3] tv_decode_angles owes for these records, in fp32 and in float64: heads = three
    (bin, offset) pairs of host [B, H, W, 4] arrays or None (roll, pitch, yaw), theta_range [3, C] with
    NaN = not decoded; the cell of a record from its flat index in column 7. NaN past counts[b]. Also the
    period of every element [B, K, 3] (NaN where none is owed)."""
    B, K = records.shape[:2]
    live = np.arange(K)[None, :] < np.asarray(counts)[:, None]
    flat = np.where(live, records[..., 7], 0).astype(np.int64)
    label, iy, ix = flat // (H * W), flat // W % H, flat % W
    bi = np.arange(B)[:, None].repeat(K, 1)
    out32 = np.full((B, K, 3), np.nan, np.float32)
    out64 = np.full((B, K, 3), np.nan, np.float64)
    period = np.full((B, K, 3), np.nan, np.float64)
    for a, pair in enumerate(heads):
        if pair is None:
            continue
        tr = np.where(live, np.asarray(theta_range, np.float32)[a][np.where(live, label, 0)], np.nan)
        b, o = pair[0][bi, iy * live, ix * live], pair[1][bi, iy * live, ix * live]
        out32[..., a] = angle_decode_ref(b, o, tr, torch.float32)
        out64[..., a] = angle_decode_ref(b, o, tr, torch.float64)
        period[..., a] = tr
    return out32, out64, period


def check_angles(got, out32, out64, period, what=""):
    """The bar of the device tests: the same NaN pattern as owed, and on every other element the circular
    distance (modulo the element's period) to the float64 restatement at most max(4 * e_ref, 2^-20), e_ref
    the fp32 restatement's own worst distance to float64 over this case. Returns (worst, e_ref)."""
    got = np.asarray(got)
    owed = ~np.isnan(out64)
    assert np.array_equal(np.isnan(got), ~owed), f"{what}: NaN pattern differs"
    if not owed.any():
        return 0.0, 0.0
    e_ref = float(circular_distance(out32[owed], out64[owed], period[owed]).max())
    worst = float(circular_distance(got[owed], out64[owed], period[owed]).max())
    bound = max(4 * e_ref, FLOOR)
    print(f"{what}: {int(owed.sum())} angles, device vs float64 {worst:.3e}, fp32 restatement vs float64 "
          f"{e_ref:.3e}, bound {bound:.3e}")
    assert worst <= bound, f"{what}: {worst:.3e} > {bound:.3e}"
    return worst, e_ref
