"""Golden fixture for the YOLACT masks at frame size (evaluate_batch.py:98-102,136-139,
yolact_node.py:135,143,184, utils/plot.py:148-152).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's own assemble_mask
(yolact/model/masks.py, torch only) and matplotlib's tab10. utils/plot.py and evaluate_batch.py import
cv2 at module level, which is not installed, so their lines are applied here in this script's own words:
the two F.interpolate calls, `mask > 0.5`, the colour `int(255 * cmap(class_id))` and the blend
`img[mask] = alpha * colour + (1 - alpha) * img[mask]` on a uint8 image, detection by detection. It
writes tests/golden/frame_masks_k4_18x22_45x70.npz: K = 4 prototypes 18 x 22, n = 5 detections, a
45 x 70 x 3 frame, both modes, class ids including one past tab10's end. Data only: the reference
source does not travel.
    python tests/golden/gen_golden_frame_masks.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from gen_golden_targets import REF_SRC

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "frame_masks_k4_18x22_45x70.npz"
K, MH, MW, N, H, W = 4, 18, 22, 5, 45, 70
CLASS_ID = [3, 0, 12, 9, 1]  # 12: past the ten colours
BOX = [(0.40, 0.35, 0.70, 0.60), (0.60, 0.70, 0.70, 0.55), (0.50, 0.50, 1.10, 1.10), (0.10, 0.50, 0.25, 0.90),
       (0.55, 0.08, 0.80, 0.20)]


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_SRC)
    import matplotlib
    from tauv_vision.yolact.model.masks import assemble_mask
    g = torch.Generator().manual_seed(20)
    field = torch.randn((K, 5, 6), generator=g) * 1.5
    proto = F.interpolate(field.unsqueeze(0), (MH, MW), mode="bicubic", align_corners=False).squeeze(0).contiguous()
    coeff = torch.tanh(torch.randn((N, K), generator=g) * 1.5)
    box = torch.tensor(BOX, dtype=torch.float32)
    frame = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).numpy()
    mask = assemble_mask(proto, coeff, box)
    out = dict(proto=proto.numpy(), coeff=coeff.numpy(), box=box.numpy(), mask=mask.numpy(), frame=frame,
               class_id=np.array(CLASS_ID, dtype=np.int64))
    cmap = matplotlib.colormaps.get_cmap("tab10")
    for mode in ("bilinear", "nearest"):
        if mode == "bilinear":
            up = F.interpolate(mask.unsqueeze(0), (H, W), mode="bilinear").squeeze(0)  # evaluate_batch.py:101
        else:
            up = F.interpolate(mask.unsqueeze(0), (H, W)).squeeze(0)                   # yolact_node.py:135
        # a pixel within rounding of the threshold would make the stored bits depend on the host's
        # vector width: the seed keeps the bilinear values clear of it
        assert mode == "nearest" or float((up - 0.5).abs().min()) > 1e-5, float((up - 0.5).abs().min())
        sel = (up > 0.5).numpy()
        vis = frame.copy()
        for d in range(N):
            color = cmap(int(CLASS_ID[d]))
            color = (255 * np.array(color)[:3])
            color = (int(color[0]), int(color[1]), int(color[2]))
            alpha = 0.5
            vis[sel[d]] = alpha * np.array(color) + (1 - alpha) * (vis[sel[d]])
        out["sel_" + mode] = np.packbits(sel, axis=-1)
        out["overlay_" + mode] = vis
        print(mode, "area", sel.reshape(N, -1).sum(1).tolist())
    np.savez_compressed(os.path.join(HERE, NAME), **out)
    print(NAME, os.path.getsize(os.path.join(HERE, NAME)), "bytes")


if __name__ == "__main__":
    main()
