"""Two decodes of the same (B, C, H, W, K) inside one _records_many call: decode_keypoints with as many
keypoint channels as labels and keypoint_n_detections == n_detections. Each must get its own decoder output
and host buffer — with one shared cache entry the keypoint decode overwrote the object records before the
single synchronisation, and decode_keypoints returned the keypoints as the objects."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, C, H, W, K = 2, 2, 6, 9, 5


def _prediction():
    from tauv_vision_amd.centernet import Prediction
    g = torch.Generator().manual_seed(5)
    f = {k: None for k in Prediction.__dataclass_fields__}
    f["heatmap"] = torch.randn((B, C, H, W), generator=g)
    f["keypoint_heatmap"] = torch.randn((B, C, H, W), generator=g)  # other peaks than the objects'
    f["keypoint_affinity"] = torch.randn((B, C, 2, H, W), generator=g)
    f["size"] = torch.rand((B, H, W, 2), generator=g)
    f["offset"] = torch.rand((B, H, W, 2), generator=g)
    f["depth"] = torch.randn((B, H, W, 1), generator=g)
    return Prediction(**{k: None if v is None else v.cuda() for k, v in f.items()})


def _calls(pred, mc):
    obj = (pred.heatmap, pred.size, None, pred.depth, K, 1, mc.downsample_ratio, mc.in_h, mc.in_w, 0.3, None)
    kp = (pred.keypoint_heatmap, pred.size, None, None, K, 1, mc.downsample_ratio, mc.in_h, mc.in_w, 0.3,
          pred.keypoint_affinity)
    return obj, kp


def test_two_decodes_of_one_shape_keep_their_own_records():
    import tauv_vision_amd as tv
    tvd = sys.modules["tauv_vision_amd.decode"]
    pred, mc = _prediction(), tv.ModelConfig([1], [1], 4 * H, 4 * W, 2, 1.0)
    obj, kp = _calls(pred, mc)
    want_obj, want_kp = tvd._records(*obj), tvd._records(*kp)
    assert not np.array_equal(want_obj[0], want_kp[0], equal_nan=True), "the two decodes must differ for this test"
    got_obj, got_kp = tvd._records_many([obj, kp])
    for got, want, what in ((got_obj, want_obj, "objects"), (got_kp, want_kp, "keypoints")):
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]), what
    # and in the other order, from the now warm cache
    got_kp, got_obj = tvd._records_many([kp, obj])
    assert np.array_equal(got_obj[0], want_obj[0], equal_nan=True) and np.array_equal(got_kp[0], want_kp[0],
                                                                                      equal_nan=True)


def test_decode_keypoints_with_equal_label_and_keypoint_counts():
    import tauv_vision_amd as tv
    tvd = sys.modules["tauv_vision_amd.decode"]
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), True, True,
                                             [(0.0, 0.0, 0.0)]) for i in range(C)])
    assert oc.n_labels == oc.n_keypoints == C
    pred, mc = _prediction(), tv.ModelConfig([1], [1], 4 * H, 4 * W, 2, 1.0)
    obj, kp = _calls(pred, mc)
    (rec, cnt), (krec, kcnt) = tvd._records(*obj), tvd._records(*kp)
    assert cnt.min() >= 2 and kcnt.min() >= 2
    dets = tv.decode_keypoints(pred, mc, oc, None, K, K, 0.3, 0.3, 0.0)
    assert [len(d) for d in dets] == cnt.tolist()
    for b in range(B):
        for d, r in zip(dets[b], rec[b]):
            assert (d.label, d.score, d.y, d.x, d.h, d.w, d.depth) == (int(r[0]), *[float(v) for v in r[1:7]])
        # every matched keypoint is one of the keypoint decode's records
        kps = {(float(r[2]), float(r[3])) for r in krec[b, :kcnt[b]]}
        matched = [k for d in dets[b] for k in d.keypoints if k is not None]
        assert matched and all(k in kps for k in matched)
