"""numpy restatement of the augmentation's pixel definition (tv_augment_frames in
include/tauv_vision_amd.h), written from the definition and not from the kernel. `dtype` is the
precision of every floating-point step: np.float32 evaluates each operation in fp32 in the order the
definition writes it; np.float64 is the same expression tree in double on the same fp32 records. The
difference of the two is the reference's own error e_ref, from which the GPU tests derive their band.
Philox4x32-10 is integer-exact in both."""
import numpy as np

REC = 32
MASK_VALUE = 254
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two ints -> four uint32 arrays (Salmon et al., SC'11)."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniforms(out, dtype):
    """u = ((o >> 8) + 0.5) 2^-24 in `dtype` (fp32: the sum rounds to nearest even above 2^23, the same
    way on every IEEE machine)."""
    return [((o >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24) for o in out]


def normals(frames, H, W, seed, dtype):
    """n [len(frames), 3, H, W] for counter (x, y, b, 0), key = seed: Box-Muller as the definition writes it."""
    b, y, x = np.meshgrid(np.asarray(frames), np.arange(H), np.arange(W), indexing="ij")
    o = philox4x32_10((x, y, b, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u0, u1, u2, u3 = uniforms(o, dtype)
    two_pi = dtype(np.float32(6.2831855)) if dtype is np.float32 else dtype(2 * np.pi)
    ra, rb = np.sqrt(dtype(-2) * np.log(u0)), np.sqrt(dtype(-2) * np.log(u2))
    aa, ab = two_pi * u1, two_pi * u3
    return np.stack([ra * np.cos(aa), ra * np.sin(aa), rb * np.cos(ab)], 1).astype(dtype)


def _fma(a, b, c, dtype):
    if dtype is np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def coordinates(rec, dst_hw, src_hw, dtype):
    """u, v, w, inside [Hd, Wd] of one record, in `dtype`."""
    Hd, Wd = dst_hw
    Hs, Ws = src_hw
    m = rec[:9].astype(dtype)
    Y, X = np.meshgrid(np.arange(Hd).astype(dtype) + dtype(0.5), np.arange(Wd).astype(dtype) + dtype(0.5),
                       indexing="ij")
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (m[6] * X + m[7] * Y) + m[8]
        u = ((m[0] * X + m[1] * Y) + m[2]) / w
        v = ((m[3] * X + m[4] * Y) + m[5]) / w
        inside = (w > 0) & (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
    return u, v, w, inside


def _taps(src, n, dtype):
    src = np.maximum(src, dtype(0))
    i0 = np.minimum(src.astype(np.int64), n - 1)
    l1 = np.clip(src - i0.astype(dtype), dtype(0), dtype(1))
    l0 = dtype(1) - l1
    i1 = i0 + (i0 < n - 1)
    return i0, i1, l0, l1


def _clamp255(x, dtype):
    return np.clip(x, dtype(0), dtype(255))


def _gray_consts(dtype):
    # the kernel's constants are the fp32 roundings of 0.299, 0.587, 0.114; the float64 run uses the same
    # values (it restates the same function in higher precision, not another function)
    return [dtype(np.float32(c)) for c in (0.299, 0.587, 0.114)]


def gray(r, g, b, dtype):
    c = _gray_consts(dtype)
    return (c[0] * r + c[1] * g) + c[2] * b


def gray_mean(frame_u8, rec, dtype):
    """mu_b: the mean over the whole source frame of gray(clamp(brightness perm(src)))."""
    perm = [int(np.clip(int(p), 0, 2)) for p in rec[9:12]]
    br = dtype(rec[12])
    ch = [_clamp255(frame_u8[..., p].astype(dtype) * br, dtype) for p in perm]
    return dtype(gray(ch[0], ch[1], ch[2], dtype).astype(np.float64).mean())


def pixels_before_blur(frame_u8, seg_u8, rec, b, seed, dst_hw, dtype):
    """Steps 1-5 for one frame: p [3, Hd, Wd] (0 outside), inside [Hd, Wd], seg_out [Hd, Wd]."""
    Hs, Ws = frame_u8.shape[:2]
    Hd, Wd = dst_hw
    u, v, w, inside = coordinates(rec, dst_hw, (Hs, Ws), dtype)
    us, vs = np.where(inside, u, dtype(0)), np.where(inside, v, dtype(0))
    seg_out = np.full((Hd, Wd), MASK_VALUE, np.uint8)
    if seg_u8 is not None:
        seg_out = np.where(inside, seg_u8[np.floor(vs).astype(np.int64), np.floor(us).astype(np.int64)], MASK_VALUE) \
            .astype(np.uint8)
    x0, x1, wx0, wx1 = _taps(us - dtype(0.5), Ws, dtype)
    y0, y1, wy0, wy1 = _taps(vs - dtype(0.5), Hs, dtype)
    f = frame_u8.astype(dtype)
    t = []
    for ch in range(3):
        tl, tr, bl, br_ = f[y0, x0, ch], f[y0, x1, ch], f[y1, x0, ch], f[y1, x1, ch]
        t0 = _fma(tl, wx0, tr * wx1, dtype)
        t1 = _fma(bl, wx0, br_ * wx1, dtype)
        t.append(_fma(t0, wy0, t1 * wy1, dtype))
    perm = [int(np.clip(int(p), 0, 2)) for p in rec[9:12]]
    c = [t[p] for p in perm]
    brightness, contrast, saturation, hue, sat_shift, val_shift, sigma = (dtype(rec[i]) for i in range(12, 19))
    c = [_clamp255(x * brightness, dtype) for x in c]
    if contrast != 1:
        o = (dtype(1) - contrast) * gray_mean(frame_u8, rec, dtype)
        c = [_clamp255(contrast * x + o, dtype) for x in c]
    if saturation != 1:
        o = (dtype(1) - saturation) * gray(c[0], c[1], c[2], dtype)
        c = [_clamp255(saturation * x + o, dtype) for x in c]
    if hue != 0 or sat_shift != 0 or val_shift != 0:
        rn, gn, bn = (x / dtype(255) for x in c)
        mx, mn = np.maximum(rn, np.maximum(gn, bn)), np.minimum(rn, np.minimum(gn, bn))
        d = mx - mn
        ds = np.where(d > 0, d, dtype(1))
        h = np.where(mx == rn, (gn - bn) / ds, np.where(mx == gn, (bn - rn) / ds + dtype(2), (rn - gn) / ds + dtype(4)))
        h = np.where(d > 0, h / dtype(6), dtype(0))
        s = np.where(mx > 0, d / np.where(mx > 0, mx, dtype(1)), dtype(0))
        h = h + hue
        h = h - np.floor(h)
        s = np.clip(s + sat_shift, dtype(0), dtype(1))
        val = np.clip(mx + val_shift, dtype(0), dtype(1))
        h6, vs_ = h * dtype(6), val * s
        out = []
        for i in range(3):
            kk = dtype(5 - 2 * i) + h6
            kk = np.where(kk >= 6, kk - dtype(6), kk)
            kk = np.where(kk >= 6, kk - dtype(6), kk)
            fch = np.maximum(dtype(0), np.minimum(np.minimum(kk, dtype(4) - kk), dtype(1)))
            out.append((val - vs_ * fch) * dtype(255))
        c = out
    if sigma != 0:
        n = normals([b], Hd, Wd, seed, dtype)[0]
        c = [_clamp255(x + sigma * n[i], dtype) for i, x in enumerate(c)]
    p = np.stack([np.where(inside, x, dtype(0)) for x in c]).astype(dtype)
    return p, inside, seg_out


def augment(frames_u8, seg_u8, records, seed, mean, std, dst_hw, dtype=np.float64):
    """-> img [B, 3, Hd, Wd] in `dtype`, seg_out [B, Hd, Wd] uint8, inside [B, Hd, Wd] bool."""
    frames_u8, records = np.asarray(frames_u8), np.asarray(records, dtype=np.float32)
    B = frames_u8.shape[0]
    Hd, Wd = dst_hw
    imgs, segs, ins = [], [], []
    for b in range(B):
        rec = records[b]
        p, inside, seg_out = pixels_before_blur(frames_u8[b], None if seg_u8 is None else np.asarray(seg_u8)[b], rec, b,
                                                seed, dst_hw, dtype)
        k = min(max(int(rec[19]), 1), 7) | 1
        if k > min(Hd, Wd):
            raise ValueError("blur_k exceeds the destination")
        if k > 1:
            h = k // 2
            pad = np.pad(p, ((0, 0), (h, h), (h, h)), mode="reflect")
            row = pad[:, :, 0:Wd].copy()
            for t in range(1, k):
                row = row + pad[:, :, t:t + Wd]
            acc = row[:, 0:Hd].copy()
            for t in range(1, k):
                acc = acc + row[:, t:t + Hd]
            q = acc / dtype(k * k)
        else:
            q = p
        q = np.where(inside[None], q, dtype(0)).astype(dtype)
        m = np.asarray(mean, np.float32).astype(dtype).reshape(3, 1, 1)
        s = np.asarray(std, np.float32).astype(dtype).reshape(3, 1, 1)
        imgs.append((q / dtype(255) - m) / s)
        segs.append(seg_out)
        ins.append(inside)
    return np.stack(imgs).astype(dtype), np.stack(segs), np.stack(ins)
