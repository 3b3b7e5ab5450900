"""tauv_vision_amd.yolact_loss (csrc/yolact_loss.hip) on the GPU against the reference's own results
(tests/golden/yolact_loss_*.npz) and the float64 restatement of the reference's loss
(tests/yolact_loss_ref.py), on the cases of tests/yolact_loss_cases.py: A tiny, B past one workgroup in
every kernel and off every alignment (1122 anchors, 23 x 37 prototypes from a 90 x 150 input, P = 32),
C an odd P with one truth, D no positive, E positives whose truth does not occur in the seg map.

Sets: match_index at positives, positive, negative and selected are exactly the reference's.
Tolerances (the rule of test_gpu_centernet_loss.py; none fixed from what the device gives):
  values     |T_dev - T64| <= max(4 e_ref, 2^-20) S with e_ref = |T_ref - T64| / S the reference's own fp32
             error on the same inputs and S the sum of the absolute values of the elements the term sums. The
             factor 4 covers the device's expf / logf (not libm's) and another summation order; the floor
             of 16 fp32 ulp covers the chain of rounded operations per element, so that an accidentally
             tiny e_ref stays meetable.
  gradients  per tensor max|g_dev - g64| <= max(4 max|g_ref - g64|, 2^-20 max|g64|), and exact zeros at
             non-selected anchors (classification), non-positive anchors (box_encoding, mask_coeff) and in
             the prototypes of a sample without a positive.
The measured ratios (error over tolerance, 1 is the limit) go through helpers.record_measurement;
profiles/loss/yolact_parity.json is such a record from an MI355X.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yolact_loss_cases as C
import yolact_loss_ref as R
from helpers import record_measurement

pytestmark = pytest.mark.gpu

A = "yolact_loss_a"


def on_gpu(inputs, requires_grad=True):
    return R.prediction_of(inputs, torch.float32, "cuda", requires_grad), R.truth_of(inputs, "cuda")


@functools.lru_cache(maxsize=None)
def launched(name):
    """(values, grads, sets) of one loss_with_state() call and its total.backward() on a fixture's stored
    inputs, as numpy. Computed once per case and shared; do not modify."""
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case(name)
    pred, truth = on_gpu(inputs)
    total, terms, state = L.loss_with_state(pred, truth, cfg)
    vals = dict(zip(R.TERMS, (total,) + tuple(terms)))
    for t, v in vals.items():
        assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32, t
    total.backward()
    grads = {}
    for k, t in zip(C.PREDICTION, pred):
        if k == "anchor":
            assert t.grad is None
        else:
            assert t.grad.shape == t.shape and t.grad.dtype == torch.float32, k
            grads[k] = t.grad
    want_dtype = dict(match_index=torch.int32, positive=torch.uint8, negative=torch.uint8, selected=torch.uint8)
    for k in R.SETS:
        t = getattr(state, k)
        assert t.is_cuda and t.dtype == want_dtype[k] and tuple(t.shape) == tuple(pred[0].shape[:2]), k
    return R._numpy(vals), R._numpy(grads), {k: getattr(state, k).cpu().numpy() for k in R.SETS}


@pytest.mark.parametrize("name", R.CASES)
def test_sets_are_exactly_the_reference_s(name):
    g = R.load_case(name)[0]
    sets = launched(name)[2]
    pos = g["positive"].astype(bool)
    for k in ("positive", "negative", "selected"):
        np.testing.assert_array_equal(sets[k], g[k], err_msg=k)
    np.testing.assert_array_equal(sets["match_index"][pos], g["match_index"][pos])
    assert ((sets["match_index"] >= 0) & (sets["match_index"] < g["in_truth_valid"].shape[1])).all()


@pytest.mark.parametrize("name", R.CASES)
def test_values(name):
    v64, S, g64, st, v32, g32 = R.restated(name)
    worst = R.check_values(launched(name)[0], v64, S, v32)
    record_measurement(f"yolact_loss/{name}/values", worst)
    if name == "yolact_loss_d":
        assert all(v == 0.0 for v in launched(name)[0].values())


@pytest.mark.parametrize("name", R.CASES)
def test_gradients(name):
    v64, S, g64, st, v32, g32 = R.restated(name)
    g = R.load_case(name)[0]
    worst = R.check_grads(launched(name)[1], g64, g32, g["positive"].astype(bool), g["selected"].astype(bool))
    record_measurement(f"yolact_loss/{name}/gradients", worst)
    if name == "yolact_loss_d":
        assert all(not v.any() for v in launched(name)[1].values())


def test_uint8_truth_and_host_truth_go_in():
    """The reference's train.py passes uint8 classifications and seg maps; host truth is moved over."""
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case(A)
    pred, _ = on_gpu(inputs, requires_grad=False)
    for truth in (R.truth_of({**inputs, "truth_classification": inputs["truth_classification"].to(torch.uint8)}),
                  R.truth_of({**inputs, "truth_seg_map": inputs["truth_seg_map"].long()}, "cuda"),
                  R.truth_of({**inputs, "truth_seg_map": inputs["truth_seg_map"].int()})):
        total, terms = L.loss(pred, truth, cfg)
        assert float(total) == launched(A)[0]["total"] and float(terms[2]) == launched(A)[0]["mask"]


def test_permuted_strides_bit_equal_and_nothing_copied(monkeypatch):
    """classification as a permuted view of [B, C, A] and mask_prototype as a permuted view of [B, h, w, P]
    (the prototype net's NHWC output): the same bits as the contiguous run, the views' own data_ptr and
    strides handed to the library."""
    from tauv_vision_amd import yolact_loss as L
    calls, run = [], L._Call.run
    monkeypatch.setattr(L._Call, "run", lambda self, tensors, want: (calls.append((self, tensors)), run(self, tensors, want))[1])
    for name in (A, "yolact_loss_b"):
        g, c, cfg, inputs = R.load_case(name)
        pred, truth = on_gpu(inputs)
        cls_base = pred[0].detach().permute(0, 2, 1).contiguous().requires_grad_(True)
        proto_base = pred[4].detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        cls, proto = cls_base.permute(0, 2, 1), proto_base.permute(0, 3, 1, 2)
        assert not cls.is_contiguous() and not proto.is_contiguous()
        total, terms = L.loss((cls, pred[1], pred[2], pred[3], proto), truth, cfg)
        total.backward()
        vals, grads, _ = launched(name)
        assert float(total.detach()) == vals["total"] and [float(t.detach()) for t in terms] == [vals[t] for t in R.TERMS[1:]]
        np.testing.assert_array_equal(cls_base.grad.permute(0, 2, 1).double().cpu().numpy(), grads["classification"])
        np.testing.assert_array_equal(proto_base.grad.permute(0, 3, 1, 2).double().cpu().numpy(), grads["mask_prototype"])
        np.testing.assert_array_equal(pred[2].grad.double().cpu().numpy(), grads["mask_coeff"])
        call, tensors = calls[-1]
        d = call.desc
        assert tensors[0].data_ptr() == cls.data_ptr() and tensors[3].data_ptr() == proto.data_ptr()
        assert d.classification == cls_base.data_ptr() and tuple(d.classification_stride) == cls.stride()
        assert d.mask_prototype == proto_base.data_ptr() and tuple(d.mask_prototype_stride) == proto.stride()


def test_two_calls_bit_equal_on_dirty_buffers(monkeypatch):
    """The second call gets every buffer it allocates (gradients, sets, workspace, outputs) prefilled with
    0x5A: each byte it returns was written by the call."""
    from tauv_vision_amd import yolact_loss as L
    empty, empty_like = torch.empty, torch.empty_like

    def dirty(make):
        def f(*a, **k):
            t = make(*a, **k)
            if t.is_cuda:
                torch.as_strided(t, (t.numel(),), (1,)).view(torch.uint8).fill_(0x5A)
            return t
        return f
    for name in ("yolact_loss_b", "yolact_loss_d", "yolact_loss_e"):
        first = launched(name)
        g, c, cfg, inputs = R.load_case(name)
        pred, truth = on_gpu(inputs)
        monkeypatch.setattr(torch, "empty", dirty(empty))
        monkeypatch.setattr(torch, "empty_like", dirty(empty_like))
        total, terms, state = L.loss_with_state(pred, truth, cfg)
        total.backward()
        monkeypatch.undo()
        for t, v in zip(R.TERMS, (total,) + tuple(terms)):
            assert float(v) == first[0][t], (name, t)
        for k, t in zip(C.PREDICTION, pred):
            if k != "anchor":
                np.testing.assert_array_equal(t.grad.double().cpu().numpy(), first[1][k], err_msg=k)
        pos = first[2]["positive"].astype(bool)
        for k in ("positive", "negative", "selected"):
            np.testing.assert_array_equal(getattr(state, k).cpu().numpy(), first[2][k], err_msg=k)
        np.testing.assert_array_equal(state.match_index.cpu().numpy()[pos], first[2]["match_index"][pos])


def test_no_grad_allocates_no_gradient_buffer():
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case("yolact_loss_b")
    pred, truth = on_gpu(inputs)
    grad_bytes = sum(t.numel() * 4 for k, t in zip(C.PREDICTION, pred) if k != "anchor")
    with torch.no_grad():
        L.loss(pred, truth, cfg)  # the library is loaded, the allocator warm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        total, terms = L.loss(pred, truth, cfg)
        assert torch.cuda.max_memory_allocated() - before < grad_bytes // 4
    assert not total.requires_grad and float(total) == launched("yolact_loss_b")[0]["total"]
    # nothing requires grad: the same
    pred, truth = on_gpu(inputs, requires_grad=False)
    total, _ = L.loss(pred, truth, cfg)
    assert not total.requires_grad and float(total) == launched("yolact_loss_b")[0]["total"]


def _head(inputs, dtype, dev):
    """mask_coeff from a Linear, mask_prototype from a 1x1 Conv2d, seeded. -> (modules, prediction builder)."""
    gen = torch.Generator().manual_seed(7)
    B, Aa, P = inputs["mask_coeff"].shape
    h, w = inputs["mask_prototype"].shape[2:]
    x_c = torch.randn((B, Aa, 6), generator=gen)
    x_p = torch.randn((B, 4, h, w), generator=gen)
    w_l, w_c = 0.4 * torch.randn((P, 6), generator=gen), 0.8 * torch.randn((P, 4, 1, 1), generator=gen)
    lin, conv = torch.nn.Linear(6, P).to(dev, dtype), torch.nn.Conv2d(4, P, 1).to(dev, dtype)
    with torch.no_grad():
        lin.weight.copy_(w_l)
        lin.bias.zero_()
        conv.weight.copy_(w_c)
        conv.bias.fill_(0.1)

    def prediction():
        f = lambda k: inputs[k].to(dev, dtype)  # noqa: E731
        return (f("classification"), f("box_encoding"), torch.tanh(lin(x_c.to(dev, dtype))), f("anchor"),
                torch.relu(conv(x_p.to(dev, dtype))))
    return (lin, conv), prediction


def test_drop_in_linear_and_conv_heads():
    """A Linear produces mask_coeff and a Conv2d the prototypes; total.backward() reaches their weights,
    within the gradient rule of the restatement's (float64 against fp32, both on the CPU)."""
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case(A)

    def weight_grads(dtype, dev, fn):
        mods, prediction = _head(inputs, dtype, dev)
        fn(prediction(), R.truth_of(inputs, dev)).backward()
        return [m.weight.grad.double().cpu().numpy() for m in mods]
    ref = lambda dtype: weight_grads(dtype, "cpu", lambda p, t: R.loss_ref(p, t, cfg)[0]["total"])  # noqa: E731
    w64, w32 = ref(torch.float64), ref(torch.float32)
    wdev = weight_grads(torch.float32, "cuda", lambda p, t: L.loss(p, t, cfg)[0])
    for name, d, a, r in zip(("linear", "conv"), wdev, w64, w32):
        bound = max(4 * np.abs(r - a).max(), R.FLOOR * np.abs(a).max())
        err = np.abs(d - a).max()
        print(f"{name} weight grad: max error {err:.3g} bound {bound:.3g}")
        record_measurement(f"yolact_loss/drop_in/{name}", err / bound)
        assert np.abs(a).max() > 0 and err <= bound, name


def test_backward_through_the_mask_term_alone():
    """mask_loss.backward() gives mask_coeff and mask_prototype the mask term's gradients (total's, which
    have no other source) and zeros to classification and box_encoding; a second backward raises."""
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case(A)
    pred, truth = on_gpu(inputs)
    total, terms = L.loss(pred, truth, cfg)
    terms[2].backward()
    grads = launched(A)[1]
    assert not pred[0].grad.any() and not pred[1].grad.any()
    np.testing.assert_array_equal(pred[2].grad.double().cpu().numpy(), grads["mask_coeff"])
    np.testing.assert_array_equal(pred[4].grad.double().cpu().numpy(), grads["mask_prototype"])
    assert np.abs(grads["mask_coeff"]).max() > 0 and np.abs(grads["mask_prototype"]).max() > 0
    with pytest.raises(RuntimeError):
        total.backward()


def test_more_mined_than_negatives_mines_every_negative():
    """The departure: ratio * n_positive > n_negative mines every negative and nothing else, and does not
    raise (the reference's topk would go on into neutral and positive anchors, or raise for k > A)."""
    from tauv_vision_amd import yolact_loss as L
    g, c, cfg, inputs = R.load_case(A)
    pos, neg = g["positive"].astype(bool), g["negative"].astype(bool)
    ratio = 400
    assert (ratio * pos.sum(axis=1) > neg.sum(axis=1)).all() and (~(pos | neg)).any()
    pred, truth = on_gpu(inputs)
    total, terms, state = L.loss_with_state(pred, truth, SimpleNamespace(**{**vars(cfg), "negative_example_ratio": ratio}))
    total.backward()
    np.testing.assert_array_equal(state.selected.cpu().numpy().astype(bool), pos | neg)
    # the classification term over that set, divided by (1 + ratio) * n_positive
    logp = torch.log_softmax(inputs["classification"].double(), dim=-1)
    target = torch.where(torch.from_numpy(pos), torch.gather(inputs["truth_classification"], 1,
                                                             torch.from_numpy(g["match_index"]).clamp(min=0).long()), 0)
    ce = -torch.gather(logp, 2, target.unsqueeze(-1)).squeeze(-1)
    want = float(ce[torch.from_numpy(pos | neg)].sum()) / ((1 + ratio) * int(pos.sum()))
    assert abs(float(terms[0]) - want) <= R.FLOOR * want  # the values' floor: every summed element is positive
    assert not pred[0].grad[~torch.from_numpy(pos | neg).cuda()].any()
    assert float(terms[1]) == launched(A)[0]["box"] and float(terms[2]) == launched(A)[0]["mask"]


def test_refusals_launch_nothing(monkeypatch):
    from tauv_vision_amd import _lib, yolact_loss as L
    g, c, cfg, inputs = R.load_case(A)
    pred, truth = on_gpu(inputs)
    _lib.lib()

    def no_launch():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "lib", no_launch)

    def refused(exc, match, pred=pred, truth=truth, cfg=cfg):
        with pytest.raises(exc, match=match):
            L.loss(pred, truth, cfg)
    refused(ValueError, "on the host", pred=(pred[0], pred[1].detach().cpu(), *pred[2:]))
    refused(ValueError, "refused", pred=(pred[0].detach().half(), *pred[1:]))
    refused(ValueError, "refused", pred=(*pred[:4], pred[4].detach().bfloat16()))
    refused(ValueError, "expected", pred=(pred[0], pred[1][:, :-1], *pred[2:]))
    refused(ValueError, "expected", pred=(*pred[:2], pred[2][:1], *pred[3:]))
    refused(ValueError, "expected", pred=(*pred[:4], pred[4][:, :-1]))
    refused(ValueError, "T == 0", truth=(truth[0][:, :0], truth[1][:, :0], truth[2][:, :0], *truth[3:]))
    refused(ValueError, "negative_example_ratio", cfg=SimpleNamespace(**{**vars(cfg), "negative_example_ratio": -2}))
    bad = truth[1].clone()
    bad[0, 0] = pred[0].shape[2]
    refused(IndexError, "out of range", truth=(truth[0], bad, *truth[2:]))


def test_c_abi_rejects_bad_arguments():
    """TV_EINVAL with nothing written: a null description, pointer or workspace, a short workspace, T = 0,
    P = 0, a negative ratio, some but not all gradient buffers."""
    from tauv_vision_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = ctypes.c_void_p(buf.data_ptr()), _lib.stream_of(buf.device)
    pointers = [f[0] for f in _lib.YolactLossDesc._fields_ if f[1] is _lib.c_vp]

    def desc(**over):
        d = _lib.YolactLossDesc()
        d.B, d.A, d.C, d.P, d.T, d.h, d.w, d.in_h, d.in_w, d.seg_itemsize = 1, 8, 2, 4, 2, 4, 4, 8, 8, 1
        d.negative_example_ratio, d.iou_pos_threshold, d.iou_neg_threshold = 3, 0.5, 0.4
        d.box_variances[:] = [0.1, 0.2]
        for f in pointers:
            setattr(d, f, buf.data_ptr())
        for n in ("classification", "box_encoding", "mask_coeff"):
            getattr(d, n + "_stride")[:] = [32, 4, 1]
            getattr(d, "grad_" + n + "_stride")[:] = [32, 4, 1]
        d.anchor_stride[:] = [4, 1]
        d.mask_prototype_stride[:] = [64, 16, 4, 1]
        d.grad_mask_prototype_stride[:] = [64, 16, 4, 1]
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def calls(d, ws=p, n=buf.numel() * 4):
        ref = ctypes.byref(d) if d is not None else None
        return [getattr(lib, "tv_yolact_loss_" + st)(ref, ws, n, s) for st in _lib.YOLACT_LOSS_STAGES] + \
            [lib.tv_yolact_loss_finalize(ref, ws, n, p, s)]

    size = ctypes.c_int64()
    assert lib.tv_yolact_loss_workspace_size(ctypes.byref(desc()), ctypes.byref(size)) == _lib.TV_OK and size.value > 0
    assert size.value <= buf.numel() * 4
    bad = [desc(T=0), desc(P=0), desc(B=0), desc(A=0), desc(C=0), desc(h=0), desc(in_w=0), desc(seg_itemsize=3),
           desc(negative_example_ratio=-1), desc(grad_mask_coeff=None)]
    bad += [desc(**{f: None}) for f in pointers if not f.startswith("grad_")]
    d = desc()
    d.mask_prototype_stride[1] = -16
    bad.append(d)
    for d in bad:
        assert calls(d) == [_lib.TV_EINVAL] * 7
        assert lib.tv_yolact_loss_workspace_size(ctypes.byref(d), ctypes.byref(size)) == _lib.TV_EINVAL
    assert calls(None) == [_lib.TV_EINVAL] * 7
    assert calls(desc(), ws=None) == [_lib.TV_EINVAL] * 7
    lib.tv_yolact_loss_workspace_size(ctypes.byref(desc()), ctypes.byref(size))
    assert calls(desc(), n=size.value - 1) == [_lib.TV_EINVAL] * 7
    assert lib.tv_yolact_loss_finalize(ctypes.byref(desc()), p, size.value, None, s) == _lib.TV_EINVAL
    no_grads = desc(grad_classification=None, grad_box_encoding=None, grad_mask_coeff=None, grad_mask_prototype=None)
    assert lib.tv_yolact_loss_mask_coeff(ctypes.byref(no_grads), p, buf.numel() * 4, s) == _lib.TV_EINVAL
    assert lib.tv_yolact_loss_workspace_size(ctypes.byref(desc()), None) == _lib.TV_EINVAL
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing was launched
