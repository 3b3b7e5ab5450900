"""tests/augment_ref.py on its own: Philox4x32-10 against its published known-answer vectors, the noise
statistics within derived bounds, and the restatement's anchors against torch (identity = the oracle's
preprocess, flips = torch.flip), so that the GPU tests compare the kernel against a checked reference."""
import numpy as np
import torch

import augment_ref as R
from oracle.ref_preprocess import MEAN, STD, preprocess


def _frames(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)


def _identity_records(B, hs, ws, hd, wd):
    rec = np.zeros((B, R.REC), np.float32)
    rec[:, [0, 4, 8]] = [ws / wd, hs / hd, 1.0]
    rec[:, 9:12] = [0, 1, 2]
    rec[:, 12:15] = 1
    rec[:, 19] = 1
    return rec


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    zero = R.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = R.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2)
    assert [int(v) for v in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_philox_is_elementwise():
    x = np.arange(5, dtype=np.uint32)
    whole = R.philox4x32_10((x, 7, 2, 0), (11, 13))
    for i in range(5):
        one = R.philox4x32_10((int(x[i]), 7, 2, 0), (11, 13))
        assert [int(v[i]) for v in whole] == [int(v) for v in one]


def test_noise_statistics():
    """N = 3 B H W unclamped standard normals: the mean's standard error is 1 / sqrt(N), the variance's
    sqrt(2 / N); both bounds are six standard errors."""
    B, H, W = 3, 64, 65
    for dtype in (np.float64, np.float32):
        n = R.normals(range(B), H, W, 0x1234567890abcdef, dtype).astype(np.float64)
        N = n.size
        assert N == 3 * B * H * W
        mean, var = n.mean(), n.var()
        print(f"{dtype.__name__}: N = {N}, mean = {mean:.3e} (bound {6 / np.sqrt(N):.3e}), var - 1 = {var - 1:.3e} "
              f"(bound {6 * np.sqrt(2 / N):.3e})")
        assert abs(mean) < 6 / np.sqrt(N)
        assert abs(var - 1) < 6 * np.sqrt(2 / N)


def test_uniforms_never_reach_zero_and_agree_between_precisions():
    o = np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32)
    u32, u64 = R.uniforms([o], np.float32)[0], R.uniforms([o], np.float64)[0]
    assert (u32 > 0).all() and (u32 <= 1).all() and (u64 > 0).all() and (u64 < 1).all()
    assert np.abs(u32.astype(np.float64) - u64).max() <= 2.0 ** -25


def test_identity_is_the_oracles_preprocess_bit_for_bit():
    frames = _frames(2, 9, 11, 1)
    img, _, inside = R.augment(frames.numpy(), None, _identity_records(2, 9, 11, 9, 11), 0, MEAN, STD, (9, 11),
                               np.float32)
    assert inside.all()
    assert np.array_equal(img, preprocess(frames, 9, 11).numpy())


def test_flips_are_torch_flip():
    frames = _frames(1, 8, 10, 2)
    seg = torch.randint(0, 5, (1, 8, 10), dtype=torch.uint8)
    want = preprocess(frames, 8, 10)
    for hflip, vflip in ((1, 0), (0, 1), (1, 1)):
        rec = _identity_records(1, 8, 10, 8, 10)
        if hflip:
            rec[0, [0, 2]] = [-1, 10]
        if vflip:
            rec[0, [4, 5]] = [-1, 8]
        img, seg_out, inside = R.augment(frames.numpy(), seg.numpy(), rec, 0, MEAN, STD, (8, 10), np.float32)
        dims = [d for d, f in ((3, hflip), (2, vflip)) if f]
        assert inside.all()
        assert np.array_equal(img, torch.flip(want, dims).numpy())
        assert np.array_equal(seg_out, torch.flip(seg, [d - 1 for d in dims]).numpy())


def test_outside_is_padding_and_blur_keeps_it():
    frames = _frames(1, 8, 8, 3)
    rec = _identity_records(1, 8, 8, 8, 8)
    rec[0, 2] = 3.0  # u = X + 3: the last three columns read past the frame
    rec[0, 18], rec[0, 19] = 5.0, 3
    seg = np.ones((1, 8, 8), np.uint8)
    img, seg_out, inside = R.augment(frames.numpy(), seg, rec, 9, MEAN, STD, (8, 8), np.float64)
    assert inside[0, :, :5].all() and not inside[0, :, 5:].any()
    assert (seg_out[0, :, 5:] == R.MASK_VALUE).all() and (seg_out[0, :, :5] == 1).all()
    pad = (0 - np.asarray(MEAN, np.float32).astype(np.float64)) / np.asarray(STD, np.float32).astype(np.float64)
    assert np.array_equal(img[0, :, :, 5:], np.broadcast_to(pad.reshape(3, 1, 1), (3, 8, 3)))


def test_hue_turn_and_gray_frames():
    """hue = 1 is the identity and R = G = B pixels ignore saturation and hue, to rounding (float64)."""
    frames = _frames(1, 6, 7, 4)
    base = R.augment(frames.numpy(), None, _identity_records(1, 6, 7, 6, 7), 0, MEAN, STD, (6, 7))[0]
    rec = _identity_records(1, 6, 7, 6, 7)
    rec[0, 15] = 1.0
    assert np.abs(R.augment(frames.numpy(), None, rec, 0, MEAN, STD, (6, 7))[0] - base).max() < 1e-12
    gray = frames[..., :1].expand(-1, -1, -1, 3).contiguous()
    base = R.augment(gray.numpy(), None, _identity_records(1, 6, 7, 6, 7), 0, MEAN, STD, (6, 7))[0]
    rec = _identity_records(1, 6, 7, 6, 7)
    rec[0, 14], rec[0, 15] = 1.7, 0.3
    # the fp32 gray weights sum to 1 within 2^-24: a gray pixel moves by at most 0.7 * 255 * 2^-23 u8 units
    assert np.abs(R.augment(gray.numpy(), None, rec, 0, MEAN, STD, (6, 7))[0] - base).max() < 1e-6
