"""tauv_vision_amd.loss.loss (csrc/loss.hip) on the GPU against the float64 restatement of the reference's
loss (tests/centernet_loss_ref.py): on the fixtures the reference itself produced (tests/golden/loss_*.npz),
whose maps fit one dense workgroup per plane, and on the generated cases of tests/centernet_loss_cases.py
(rows, vec3, scal3, many), which reach the launcher's other schedules: vectors that straddle rows, three
workgroups per plane with a partly live last one on either route, 260 samples, half dtypes on the scalar
route and through NHWC slices, a misaligned heatmap. Each of those runs asserts the route it took, through
the workgroups per plane that the workspace size of the call's own description implies.

Tolerances (none fixed in advance; S and the restatement are described in centernet_loss_ref.py):
  values     |T_dev - T64| <= max(4 e_ref, 2^-20) S with e_ref = |T_ref - T64| / S the reference's own fp32
             error on the same fixture. The factor 4 covers the device's expf / logf / powf (not libm's)
             and another summation order; the floor of 16 fp32 ulp covers the chain of about eight
             rounded operations per element, so that an accidentally tiny e_ref stays meetable.
  gradients  per tensor max|g_dev - g64| <= max(4 max|g_ref - g64|, 2^-20 max|g64|); for fp16 / bf16
             inputs plus 2^-10 |g64| / 2^-7 |g64| per element, the rounding of the stored gradient.
NaN is required exactly where the reference has NaN. With half inputs the restatement runs on the
half-rounded prediction, and the fp32 side of e_ref is the fp32 restatement on that same prediction
(test_centernet_loss_ref_cpu.py shows it equals the reference bit for bit); so is the fp32 side of every
generated case. The rule itself (check_values / check_grads) lives in centernet_loss_ref.py, where
test_centernet_loss_cases_cpu.py shows that it reports a dropped workgroup, partials of the wrong kind, a
vector written one row down, a dropped sample and an ungathered object.

Measured on MI355X, generated cases (profiles/loss/generated_cases.json; worst value error over its
tolerance / worst gradient error over its bound, 1 is the limit):
  rows   fp32 0.10 / 0.25   fp16 0.25 / 0.91   bf16 0.19 / 0.89   misaligned fp32 0.10 / 0.25, fp16 0.25 / 0.91
  vec3   fp32 0.25 / 0.28   fp16 NHWC slices 0.38 / 0.81
  scal3  fp32 0.18 / 0.25   fp16 0.19 / 0.80   bf16 0.20 / 0.78
  many   fp32 0.08 / 0.25
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import centernet_loss_ref as R
from centernet_loss_ref import FLOOR, _numpy, check_grads, check_values, restated  # noqa: F401
from helpers import record_measurement

pytestmark = pytest.mark.gpu

A = "loss_allheads_b2_24x40"
DENSE = ("heatmap", "keypoint_heatmap", "keypoint_affinity")
HALF = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
# generated case: the workgroups per plane (gx) of the route it is meant to run, of the scalar route
GX = {"rows": (1, 3), "vec3": (3, 9), "scal3": (3, 3), "many": (1, 1)}


def reference_layout(pred, dtype, dev="cuda", heatmap_offset=0):
    """The reference torch model's layout: NCHW-contiguous heatmaps, NHWC views of NCHW heads.
    -> (leaves, views): the leaves require grad. With `heatmap_offset` the heatmap is a contiguous view that
    many elements into a larger buffer (its gradient is retained on the view)."""
    leaf, view = {}, {}
    for h, v in pred.items():
        if v is None:
            view[h] = None
            continue
        nchw = v if h in DENSE else v.permute(0, 3, 1, 2)
        leaf[h] = nchw.to(dev, dtype).contiguous().requires_grad_(True)
        if h == "heatmap" and heatmap_offset:
            buf = torch.zeros(v.numel() + 2 * heatmap_offset, dtype=dtype, device=dev)
            buf[heatmap_offset:heatmap_offset + v.numel()] = leaf[h].detach().reshape(-1)
            leaf[h] = buf.requires_grad_(True)[heatmap_offset:heatmap_offset + v.numel()].view(v.shape)
            leaf[h].retain_grad()
            assert leaf[h].is_contiguous() and leaf[h].data_ptr() % (4 * leaf[h].element_size())
        view[h] = leaf[h] if h in DENSE else leaf[h].permute(0, 2, 3, 1)
    return leaf, view


def leaf_grads(leaf):
    return {h: (t.grad if h in DENSE else t.grad.permute(0, 2, 3, 1)) for h, t in leaf.items()}


def cuda_truth(truth):
    from tauv_vision_amd import loss as L
    return L.PoseSample(**{k: v.cuda() for k, v in vars(truth).items()})


def nhwc_slices(pred, oc, dtype=torch.float32):
    """The prediction as channel slices of one NHWC tensor (prediction_from_nhwc).
    -> (base, views, the tauv_vision_amd object config, its channel table)."""
    from tauv_vision_amd.centernet import prediction_fields, prediction_from_nhwc
    toc = object_config_of(oc)
    fields = prediction_fields(toc)
    B, H, W = pred["size"].shape[:3]
    base = torch.zeros((B, H, W, sum(n for _, n in fields.values())))
    for h, (s, n) in fields.items():
        v = pred[h]
        v = v.permute(0, 2, 3, 1) if h in DENSE[:2] else v.permute(0, 3, 4, 1, 2).reshape(B, H, W, n) \
            if h == "keypoint_affinity" else v
        base[..., s:s + n] = v
    base = base.to("cuda", dtype).requires_grad_(True)
    return base, prediction_from_nhwc(base, toc), toc, fields


def workgroups_per_plane(desc):
    """gx of a call's description, from the workspace the library asks for:
    bytes = 4 * (4 * B * (L + K) * gx + 16 * B)."""
    from tauv_vision_amd import _lib
    n = ctypes.c_int64()
    assert _lib.lib().tv_centernet_loss_workspace_size(ctypes.byref(desc), ctypes.byref(n)) == _lib.TV_OK
    B = desc.B
    P = desc.n_labels + (desc.n_keypoints if desc.tensor[_lib.LOSS_TENSORS.index("keypoint_heatmap")].data else 0)
    floats = n.value // 4 - 16 * B
    assert n.value % 4 == 0 and floats > 0 and floats % (4 * B * P) == 0, (n.value, B, P)
    return floats // (4 * B * P)


@functools.lru_cache(maxsize=None)
def launched(name, dtype=torch.float32, layout="reference"):
    """(values, grads, gx) of one loss() call and its backward on a case, as float64 numpy; gx the dense
    workgroups per plane of the description the call handed the library. Layouts: "reference" (the
    reference model's), "misaligned" (the same with the heatmap four bytes into a larger buffer), "nhwc"
    (channel slices of one NHWC tensor; the gradients are those the loss returns for the slices)."""
    from tauv_vision_amd import loss as L
    g, mc, tc, oc, truth, pred = R.case_inputs(name)
    gx, run = [], L._Call.run

    def spy(self, tensors, want):
        out = run(self, tensors, want)
        gx.append(workgroups_per_plane(self.desc))  # while the tensors the description points to are alive
        return out
    seen = {}
    if layout == "nhwc":
        base, views, oc, _ = nhwc_slices(pred, oc, dtype)
        for h in R.HEADS:
            assert not getattr(views, h).is_contiguous()
            getattr(views, h).register_hook(lambda gr, h=h: seen.__setitem__(h, gr))
    else:
        leaf, view = reference_layout(pred, dtype, heatmap_offset=4 // dtype.itemsize if layout == "misaligned" else 0)
        views = SimpleNamespace(**view)
    L._Call.run = spy
    try:
        losses = L.loss(views, cuda_truth(truth), mc, tc, oc, None)
    finally:
        L._Call.run = run
    assert losses.heatmap is losses.total
    losses.total.backward()
    vals = {t: getattr(losses, t) for t in R.TERMS}
    present = [t for t in R.TERMS if "val_" + t in g.files] if g is not None else \
        [t for t in R.TERMS if t in restated(name)[0]]
    for t, v in vals.items():
        assert (v.dim() == 0 and v.is_cuda and v.dtype == torch.float32) == (t in present), t
    if layout != "nhwc":
        for h, t in leaf.items():
            assert t.grad.dtype == dtype and t.grad.shape == t.shape, h
        seen = leaf_grads(leaf)
    assert len(gx) == 1
    return _numpy({t: v for t, v in vals.items() if v.dim() == 0}), _numpy(seen), gx[0]


def device(name, dtype=torch.float32):
    """(values, grads) of loss() on a case in the reference's layout, as float64 numpy."""
    return launched(name, dtype)[:2]


@pytest.mark.parametrize("name", R.CASES)
def test_values(name):
    v64, S, _, v32, _ = restated(name)
    check_values(device(name)[0], v64, S, v32)


@pytest.mark.parametrize("name", R.CASES)
def test_gradients(name):
    _, _, g64, _, g32 = restated(name)
    check_grads(device(name)[1], g64, g32)
    if name.endswith("_nopositive"):  # N == 0: the keypoint-heatmap term and its gradient are zero
        assert device(name)[0]["keypoint_heatmap"] == 0.0 and not device(name)[1]["keypoint_heatmap"].any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_half_inputs(dtype):
    v64, S, g64, v32, g32 = restated(A, dtype)
    vals, grads = device(A, dtype)
    check_values(vals, v64, S, v32)
    check_grads(grads, g64, g32, HALF[dtype])


def _measured(name, dtype, layout, vals, grads):
    """Checks a generated case's run against the float64 restatement and records the worst ratios."""
    v64, S, g64, v32, g32 = restated(name, dtype)
    worst = {"values": check_values(vals, v64, S, v32), "gradients": check_grads(grads, g64, g32, HALF.get(dtype, 0.0))}
    key = f"loss/{name}/{str(dtype)[len('torch.'):]}" + ("" if layout == "reference" else "/" + layout)
    record_measurement(key, worst)
    print(key, worst)


@pytest.mark.parametrize("name,dtype", [("rows", torch.float32), ("rows", torch.float16), ("rows", torch.bfloat16),
                                        ("vec3", torch.float32), ("scal3", torch.float32), ("scal3", torch.float16),
                                        ("scal3", torch.bfloat16), ("many", torch.float32)],
                         ids=lambda v: v if isinstance(v, str) else str(v)[len("torch."):])
def test_generated_case(name, dtype):
    """A generated case (centernet_loss_cases.GENERATED) in the reference's layout, on the route it was
    made for: values and gradients against the float64 restatement."""
    vals, grads, gx = launched(name, dtype)
    assert gx == GX[name][0], (name, gx)
    _measured(name, dtype, "reference", vals, grads)


def test_generated_nhwc_slices_in_fp16():
    """vec3 in fp16 as channel slices of one NHWC tensor: the scalar route through the slices' strides. The
    per-cell arithmetic and the scale do not depend on the route: the gradients have the bits of the
    contiguous run's (vector route, three workgroups per plane)."""
    vals, grads, gx = launched("vec3", torch.float16, "nhwc")
    _, want, gx_vec = launched("vec3", torch.float16)
    assert (gx_vec, gx) == GX["vec3"]
    assert sorted(grads) == sorted(want)
    for h in want:
        np.testing.assert_array_equal(grads[h], want[h], err_msg=h)
    _measured("vec3", torch.float16, "nhwc", vals, grads)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_generated_misaligned_heatmap_leaves_the_vector_route(dtype):
    """rows with the heatmap a contiguous view four bytes (one fp32, two fp16 elements) into a larger
    buffer: vector_ok's alignment mask sends the call down the scalar route, and every gradient has the
    aligned run's bits."""
    vals, grads, gx = launched("rows", dtype, "misaligned")
    _, want, gx_vec = launched("rows", dtype)
    assert (gx_vec, gx) == GX["rows"]
    for h in want:
        np.testing.assert_array_equal(grads[h], want[h], err_msg=h)
    _measured("rows", dtype, "misaligned", vals, grads)


def object_config_of(oc):
    """A tauv_vision_amd ObjectConfigSet with the fixture's labels, angle moduli, depth and keypoint count."""
    import tauv_vision_amd as tv
    cfgs = []
    for i, c in enumerate(oc.configs):
        kps = [(0.0, 0.0, 0.0)] * oc.n_keypoints if i == 0 and oc.n_keypoints else None
        a = {x: tv.AngleConfig(getattr(c, x).modulo is not None, getattr(c, x).modulo) for x in ("yaw", "pitch", "roll")}
        cfgs.append(tv.ObjectConfig(f"o{i}", a["yaw"], a["pitch"], a["roll"], True, kps is not None, kps))
    return tv.ObjectConfigSet(cfgs)


def test_layouts_bit_equal_and_nothing_copied(monkeypatch):
    """Case A as channel slices of one NHWC tensor (prediction_from_nhwc) and in the reference model's
    layout: the same bits. The library is handed the views themselves (their data_ptr inside the one NHWC
    tensor, their strides), and each gradient comes back shaped by its own tensor's strides."""
    from tauv_vision_amd import _lib, loss as L
    calls, run = [], L._Call.run
    monkeypatch.setattr(L._Call, "run", lambda self, tensors, want: (calls.append(self), run(self, tensors, want))[1])
    g, mc, tc, oc, truth, pred = R.load_case(A)
    base, views, toc, fields = nhwc_slices(pred, oc)
    kept = {h: getattr(views, h) for h in R.HEADS}
    seen = {}  # the gradient tensors as the loss returns them, before autograd folds them into base.grad
    for h, t in kept.items():
        assert not t.is_contiguous()
        t.register_hook(lambda gr, h=h: seen.__setitem__(h, gr))
    losses = L.loss(views, cuda_truth(truth), mc, tc, toc, None)
    losses.total.backward()
    vals, grads = device(A)
    for t in R.TERMS:
        assert float(getattr(losses, t).detach().double()) == vals[t], t
    desc = calls[0].desc
    for h, t in kept.items():
        gr, e = seen[h], desc.tensor[_lib.LOSS_TENSORS.index(h)]
        np.testing.assert_array_equal(gr.double().cpu().numpy(), grads[h], err_msg=h)
        assert e.data == t.data_ptr() and tuple(e.stride[:t.dim()]) == t.stride(), h
        assert base.data_ptr() <= e.data < base.data_ptr() + base.numel() * base.element_size(), h
        assert gr.stride() == torch.empty_like(t).stride(), h
        s, n = fields[h]
        np.testing.assert_array_equal(base.grad[..., s:s + n].reshape(-1).cpu().numpy(),
                                      (gr.permute(0, 2, 3, 1) if h in DENSE[:2] else
                                       gr.permute(0, 3, 4, 1, 2) if h == "keypoint_affinity" else
                                       gr).reshape(-1).cpu().numpy(), err_msg=h)
    # the reference's layout: the permuted views of NCHW heads go in as they are
    leaf, view = reference_layout(pred, torch.float32)
    assert not view["size"].is_contiguous()
    L.loss(SimpleNamespace(**view), cuda_truth(truth), mc, tc, oc, None).total.backward()
    e = calls[1].desc.tensor[_lib.LOSS_TENSORS.index("size")]
    assert e.data == leaf["size"].data_ptr() and tuple(e.stride[:4]) == view["size"].stride()
    assert leaf["size"].grad.stride() == leaf["size"].stride()


def _second_call_on_dirty_buffers(monkeypatch, name):
    from tauv_vision_amd import loss as L
    first = device(name)
    empty, empty_like = torch.empty, torch.empty_like

    def dirty(make):
        def f(*a, **k):
            t = make(*a, **k)
            if t.is_cuda:
                torch.as_strided(t, (t.numel(),), (1,)).view(torch.uint8).fill_(0x5A)  # dense, any stride order
            return t
        return f
    monkeypatch.setattr(torch, "empty", dirty(empty))
    monkeypatch.setattr(torch, "empty_like", dirty(empty_like))
    g, mc, tc, oc, truth, pred = R.case_inputs(name)
    leaf, view = reference_layout(pred, torch.float32)
    losses = L.loss(SimpleNamespace(**view), cuda_truth(truth), mc, tc, oc, None)
    losses.total.backward()
    monkeypatch.undo()
    for t, v in first[0].items():
        assert float(getattr(losses, t).detach().double()) == v, t
    for h, v in _numpy(leaf_grads(leaf)).items():
        np.testing.assert_array_equal(v, first[1][h], err_msg=h)


def test_two_calls_bit_equal_on_dirty_buffers(monkeypatch):
    """The second call gets every buffer it allocates (gradients, partial sums, outputs) prefilled with
    0x5A: each byte it returns was written by the call."""
    _second_call_on_dirty_buffers(monkeypatch, A)


def test_generated_two_calls_bit_equal_on_dirty_buffers(monkeypatch):
    """The same on vec3: three workgroups per plane, the last one partly live."""
    _second_call_on_dirty_buffers(monkeypatch, "vec3")


def test_drop_in_conv_head():
    """A torch Conv2d produces the prediction; loss(...).total.backward() reaches its weights. With
    torch.no_grad() the call runs and allocates no gradient buffer."""
    from tauv_vision_amd import loss as L
    g, mc, tc, oc, truth, pred = R.load_case(A)
    chans = {h: (v.shape[1] * (2 if h == "keypoint_affinity" else 1) if h in DENSE else v.shape[3])
             for h, v in pred.items()}
    C, B, H, W = sum(chans.values()), pred["size"].shape[0], mc.out_h, mc.out_w
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((B, 8, H, W), generator=gen)
    w0, b0 = 0.5 * torch.randn((C, 8, 1, 1), generator=gen), torch.randn((C,), generator=gen)

    def split(out):
        p, s = {}, 0
        for h, n in chans.items():
            t = out[:, s:s + n]
            p[h] = t if h in DENSE[:2] else t.unflatten(1, (n // 2, 2)) if h == "keypoint_affinity" \
                else t.permute(0, 2, 3, 1)
            s += n
        return SimpleNamespace(**p)

    def weight_grads(dtype, dev, fn, tr):
        conv = torch.nn.Conv2d(8, C, 1).to(dev, dtype)
        with torch.no_grad():
            conv.weight.copy_(w0)
            conv.bias.copy_(b0)
        fn(split(conv(x.to(dev, dtype))), tr).backward()
        return conv.weight.grad.double().cpu().numpy(), conv.bias.grad.double().cpu().numpy()

    ref = lambda dtype: weight_grads(dtype, "cpu", lambda p, tr: R.loss_ref(p, tr, mc, tc, oc, dtype)[0]["total"], truth)  # noqa: E731
    w64, w32 = ref(torch.float64), ref(torch.float32)
    tr = cuda_truth(truth)
    wdev = weight_grads(torch.float32, "cuda", lambda p, t: L.loss(p, t, mc, tc, oc, None).total, tr)
    for name, d, a, r in zip(("weight", "bias"), wdev, w64, w32):
        bound = max(4 * np.abs(r - a).max(), FLOOR * np.abs(a).max())
        print(f"conv {name} grad: max err {np.abs(d - a).max():.3g} bound {bound:.3g}")
        assert np.abs(d - a).max() <= bound, name

    conv = torch.nn.Conv2d(8, C, 1).cuda()
    out = conv(x.cuda())
    grad_bytes = out.numel() * 4
    with torch.no_grad():
        p = split(out)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        losses = L.loss(p, tr, mc, tc, oc, None)
        assert torch.cuda.max_memory_allocated() - before < grad_bytes // 4
    assert not losses.total.requires_grad and torch.isfinite(losses.total)


def test_helper_functions():
    """focal_loss, angle_loss, depth_loss, angle_range alone, on the GPU, against the restatement's."""
    from tauv_vision_amd import loss as L
    from oracle import ref_targets as rt
    g, mc, tc, oc, truth, pred = R.load_case(A)

    def close(dev, f64, f32, what):
        f64, f32, dev = f64.double().numpy(), f32.double().numpy(), dev.double().cpu().numpy()
        bound = max(4 * np.abs(f32 - f64).max(), FLOOR * np.abs(f64).max())
        assert np.abs(dev - f64).max() <= bound, (what, np.abs(dev - f64).max(), bound)

    heat = rt.generate_heatmap(truth, mc, tc, oc.n_labels)
    prob = torch.sigmoid(pred["heatmap"])
    a, b = tc.heatmap_focal_loss_a, tc.heatmap_focal_loss_b
    close(L.focal_loss(prob.cuda(), heat.cuda(), a, b), R.focal_loss(prob.double(), heat.double(), a, b)[0],
          R.focal_loss(prob, heat, a, b)[0], "focal_loss")
    zero = torch.zeros_like(heat)
    assert float(L.focal_loss(prob.cuda(), zero.cuda(), a, b).abs().sum()) == 0.0  # N == 0: -loss_p
    B, n = truth.valid.shape
    gen = torch.Generator().manual_seed(9)
    pb, po = torch.randn((B, n, 4), generator=gen), torch.randn((B, n, 4), generator=gen)
    for k, axis in enumerate(("roll", "pitch", "yaw")):
        rng = R.angle_range(truth.label, oc, axis)
        got = L.angle_range(truth.label.cuda(), oc, L.Angle(k))
        assert got.is_cuda and torch.equal(got.cpu(), rng)
        th = getattr(truth, axis)
        close(L.angle_loss(pb.cuda(), po.cuda(), th.cuda(), got, mc.angle_bin_overlap),
              R.angle_loss(pb.double(), po.double(), th.double(), rng.double(), mc.angle_bin_overlap),
              R.angle_loss(pb, po, th, rng, mc.angle_bin_overlap), axis)
    d = torch.randn((B, n), generator=gen)
    close(L.depth_loss(d.cuda(), truth.depth.cuda()), R.depth_loss(d.double(), truth.depth.double()),
          R.depth_loss(d, truth.depth), "depth_loss")
    ang = torch.linspace(-7, 7, 29)
    assert torch.equal(L.angle_in_range(ang.cuda(), -0.5, 3.6).cpu(), R.angle_in_range(ang, -0.5, 3.6))


def test_refusals_launch_nothing(monkeypatch):
    from tauv_vision_amd import _lib, loss as L
    g, mc, tc, oc, truth, pred = R.load_case(A)
    leaf, view = reference_layout(pred, torch.float32)
    tr = cuda_truth(truth)
    _lib.lib()

    def no_launch():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "lib", no_launch)

    def refused(exc, match, view=view, tr=tr, mc=mc):
        with pytest.raises(exc, match=match):
            L.loss(SimpleNamespace(**view), tr, mc, tc, oc, None)

    refused(ValueError, "on the host", view={**view, "size": view["size"].detach().cpu()})
    refused(ValueError, "missing", tr=L.PoseSample(**{**vars(tr), "yaw": None}))
    refused(ValueError, "missing", tr=L.PoseSample(**{**vars(tr), "depth": None}))
    refused(ValueError, "the config gives", view={**view, "heatmap": view["heatmap"][:, :, :-1]})
    refused(ValueError, "the config gives", view={**view, "depth": view["depth"][..., :0]})
    refused(ValueError, "out_h/out_w", mc=SimpleNamespace(**{**vars(mc), "out_w": mc.out_w + 1}))
    refused(ValueError, "all alike", view={**view, "offset": view["offset"].detach().half()})
    refused(ValueError, "go together", view={**view, "roll_offset": None})
    refused(IndexError, "out of range", tr=L.PoseSample(**{**vars(tr), "label": tr.label + oc.n_labels}))


def test_c_abi_rejects_bad_arguments():
    """TV_EINVAL before any launch: a null description / workspace, B < 1, an empty map, a negative stride,
    a missing required head, a null truth pointer for a present head."""
    from tauv_vision_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = ctypes.c_void_p(buf.data_ptr()), _lib.stream_of(buf.device)

    def desc(**over):
        d = _lib.LossDesc()
        d.dtype, d.B, d.n_objects, d.n_labels, d.in_h, d.in_w, d.downsample_ratio = 0, 1, 2, 1, 8, 8, 2
        d.keypoint_heatmap_sigma, d.focal_alpha, d.focal_beta = 1.0, 2.0, 4.0
        for i, nd in ((0, 4), (3, 4), (4, 4)):
            d.tensor[i].data = buf.data_ptr()
            d.tensor[i].stride[:nd] = [64, 16, 4, 1]
        for f in ("valid", "label", "center", "size"):
            setattr(d, f, buf.data_ptr())
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def calls(d, ws=p, n=buf.numel() * 4):
        ref = ctypes.byref(d) if d is not None else None
        return [lib.tv_centernet_loss_dense(ref, ws, n, s), lib.tv_centernet_loss_objects(ref, ws, n, s),
                lib.tv_centernet_loss_finalize(ref, ws, n, p, s)]

    size = ctypes.c_int64()
    assert lib.tv_centernet_loss_workspace_size(ctypes.byref(desc()), ctypes.byref(size)) == _lib.TV_OK and size.value > 0
    bad = [desc(B=0), desc(in_h=1), desc(dtype=7), desc(center=None), desc(focal_alpha=0.5)]
    d = desc()
    d.tensor[3].stride[1] = -4
    bad.append(d)
    d = desc()
    d.tensor[4].data = None
    bad.append(d)
    d = desc()
    d.tensor[11].data = buf.data_ptr()  # a depth head without truth.depth
    bad.append(d)
    for d in bad:
        assert calls(d) == [_lib.TV_EINVAL] * 3
    assert calls(None) == [_lib.TV_EINVAL] * 3
    assert calls(desc(), ws=None) == [_lib.TV_EINVAL] * 3
    assert calls(desc(), n=size.value - 1) == [_lib.TV_EINVAL] * 3
    assert lib.tv_centernet_loss_finalize(ctypes.byref(desc()), p, size.value, None, s) == _lib.TV_EINVAL
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing was launched
