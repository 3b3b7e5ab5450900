"""Host restatement of what the two reference callers do with the assembled YOLACT masks (a helper,
not a test): evaluate_batch.py:98-102 (F.interpolate bilinear, > 0.5), yolact_node.py:135,143,184
(F.interpolate nearest, > 0.5) and the blend of utils/plot.py:148-152 / evaluate_batch.py:136-139,
on the CPU with torch and numpy. tests/test_frame_masks_ref_cpu.py pins it to the fixture that
tests/golden/gen_golden_frame_masks.py wrote from the reference's own assemble_mask and numpy's own
float blend; the GPU tests compare the kernel with it.

The blend is written here in integers, (pix + colour) >> 1: 0.5 colour + 0.5 pix is an integer or an
integer plus one half, exactly representable, and numpy's float64 -> uint8 assignment truncates.
"""
import numpy as np
import torch
import torch.nn.functional as F

# matplotlib's tab10 as int(255 * (v / 255)) rows (the colour the reference forms from cmap(class_id))
TAB10 = np.array([[31, 119, 180], [255, 127, 14], [44, 160, 44], [214, 39, 40], [148, 103, 189], [140, 86, 75],
                  [227, 119, 194], [127, 127, 127], [188, 189, 34], [23, 190, 207]], dtype=np.uint8)


def upsample(masks, size, mode, dtype=torch.float32):
    """masks [B, n, mh, mw] (CPU) -> F.interpolate(masks, size, mode) in `dtype`, the reference's call
    per image (mask.unsqueeze(0) is one batch entry of this)."""
    m = masks.detach().cpu().to(dtype)
    if mode == "bilinear":
        return F.interpolate(m, tuple(size), mode="bilinear")
    assert mode == "nearest"
    return F.interpolate(m, tuple(size))


def selected(masks, counts, size, mode):
    """bool [B, n, H, W]: F.interpolate(...) > 0.5 in fp32; rows at or past counts[b] are False."""
    sel = upsample(masks, size, mode) > 0.5
    for b, c in enumerate(counts):
        sel[b, int(c):] = False
    return sel


def blend(frames, sel, counts, class_id, palette=TAB10):
    """frames [B, H, W, 3] uint8 numpy, sel [B, n, H, W] bool, class_id [B, n] ints -> the frames with
    every detection d < counts[b] blended in, in order (plot.py:148-152); a class id past the palette
    takes its last row (ListedColormap)."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    sel = np.asarray(sel)
    pal = np.asarray(palette, dtype=np.uint8)
    for b in range(out.shape[0]):
        for d in range(int(counts[b])):
            colour = pal[min(max(int(class_id[b][d]), 0), len(pal) - 1)].astype(np.int32)
            m = sel[b, d]
            out[b][m] = ((out[b][m].astype(np.int32) + colour) >> 1).astype(np.uint8)
    return out


def pack(sel):
    """bool [..., H, W] numpy/torch -> uint32 numpy [..., H, ceil(W / 32)]: pixel x is bit x % 32 of word x // 32."""
    s = np.asarray(sel, dtype=bool)
    W = s.shape[-1]
    ww = (W + 31) // 32
    p = np.zeros(s.shape[:-1] + (ww * 32,), dtype=np.uint64)
    p[..., :W] = s
    p = p.reshape(s.shape[:-1] + (ww, 32))
    return (p << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def box_crop(box, mh, mw):
    """box_to_mask (boxes.py:88-103) for boxes [..., 4] (y, x, h, w) fp32 torch -> float [..., mh, mw]."""
    y = torch.arange(mh, dtype=torch.float32).view(mh, 1)
    x = torch.arange(mw, dtype=torch.float32).view(1, mw)
    b = box.to(torch.float32) * torch.tensor([mh, mw, mh, mw], dtype=torch.float32)
    b = b[..., None, None, :]
    left, right = b[..., 1] - b[..., 3] / 2, b[..., 1] + b[..., 3] / 2
    top, bottom = b[..., 0] - b[..., 2] / 2, b[..., 0] + b[..., 2] / 2
    return ((x >= left) & (x <= right) & (y >= top) & (y <= bottom)).float()


# boxes (y, x, h, w) that between them touch every image border, overlap each other, and include a
# thin and a whole-frame one; detection d of image b takes row (d + 3 b) % len
BOXES = [(0.30, 0.25, 0.62, 0.52), (0.70, 0.80, 0.62, 0.42), (0.50, 0.50, 1.20, 1.20), (0.05, 0.50, 0.12, 0.70),
         (0.95, 0.40, 0.12, 0.60), (0.50, 0.03, 0.80, 0.08), (0.45, 0.55, 0.50, 0.45), (0.60, 0.97, 0.70, 0.08)]


def synthetic_masks(B, n, mh, mw, seed):
    """(masks [B, n, mh, mw] fp32, box [B, n, 4]): sigmoid of a bicubically enlarged 5 x 6 random field,
    times the box crop — smooth blobs around 0.5 inside each box, exactly 0 outside it, as
    assemble_mask's output is."""
    g = torch.Generator().manual_seed(seed)
    field = torch.randn((B, n, 5, 6), generator=g) * 2.0
    m = torch.sigmoid(F.interpolate(field, (mh, mw), mode="bicubic", align_corners=False))
    box = torch.tensor([[BOXES[(d + 3 * b) % len(BOXES)] for d in range(n)] for b in range(B)], dtype=torch.float32)
    return (m * box_crop(box, mh, mw)).contiguous(), box
