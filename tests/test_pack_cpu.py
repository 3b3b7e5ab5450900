"""The host-only weight packer (csrc/pack.cpp) through tv_diag_pack_op: no GPU needed.

(a) Pin: tests/data/packed_weights.json holds, per (case, precision), one SHA-256 over every op's
    reported geometry, sizes and buffers in op order, and 8 hex digits per op so that a failure
    names the op. The fixture was written from the packer as it stood when the engine's single
    pack_op body had only been cut at its upload calls (no arithmetic line changed), so it pins the
    bytes the engine uploaded before the packer was split into flavours.
    When a packing change is intended, regenerate it with
        python tests/test_pack_cpu.py --regenerate
    and say in the commit which ops moved and why.
(b) Meaning: for the plain conv + BatchNorm ops of the R18-family cases the fp32 matrix is
    float32(float64(w) * scale) at [co][t * cs + ci], zero elsewhere, and the bias the folded shift.
(c) Refusals: a missing key, a wrong element count, an op index out of range.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (the suite's import paths)

from helpers import case_by_name, case_state_dict, models_index

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "packed_weights.json")
PRECISIONS = ("fp32", "fp16", "bf16")
R18_CASES = ("r18_c16_b2_96x128", "r18_c128_b1_480x640", "r18_c32_b1_96x128_allheads", "dla_var_b1_128x128")
OP_CONV = 1


def _r18(name, arch=None):
    from tauv_vision_amd.weights import ARCH_CENTERNET, ARCH_CENTERNET_BACKBONE, model_desc
    case = case_by_name(name)
    heads = [1] if arch == "backbone" else models_index()[name]["head_channels"]
    a = ARCH_CENTERNET_BACKBONE if arch == "backbone" else ARCH_CENTERNET
    return (lambda p: model_desc(case["heights"], case["channels"], case["downsamples"], heads, case["in_h"],
                                 case["in_w"], p, arch=a)), case_state_dict(name)


def _dla34():
    import dla34_layer_ref as DL
    from tauv_vision_amd.weights import dla34_desc
    return (lambda p: dla34_desc([4, 2, 2], 100, 104, p)), DL.seeded_weights()[0]


def _protonet():
    from recipe import protonet_case, protonet_inputs
    from tauv_vision_amd.weights import protonet_desc
    c = protonet_case("protonet_f64_k16_b1_9x17")
    return (lambda p: protonet_desc(c["F"], c["k"], c["H"], c["W"], p)), protonet_inputs(c)[0]


def _yolact():
    import yolact_layer_ref as YL
    from tauv_vision_amd.weights import yolact_desc
    c, sd, _, _ = YL.whole_case()
    return (lambda p: yolact_desc(c["in_h"], c["in_w"], c["F"], c["down"], c["C"], c["k"], len(c["ars"]),
                                  c["layers"], p)), sd


CASES = dict({n: (lambda n=n: _r18(n)) for n in R18_CASES},
             backbone_r18_c16_b2_96x128=lambda: _r18("r18_c16_b2_96x128", "backbone"),
             dla34_seeded_100x104=_dla34, protonet_f64_k16_b1_9x17=_protonet, yolact_whole_149x77=_yolact)
_BUILT = {}


def built(name):
    """(desc of a precision, weight views, what keeps them alive) of a case, made once."""
    if name not in _BUILT:
        from tauv_vision_amd import _lib
        desc, sd = CASES[name]()
        host = {k: v.detach().float().contiguous() for k, v in sd.items() if v.dtype.is_floating_point}
        names = [k.encode() for k in host]
        views = (_lib.WeightView * len(host))()
        for i, (k, v) in enumerate(zip(names, host.values())):
            views[i].name, views[i].data, views[i].numel = k, v.data_ptr(), v.numel()
        _BUILT[name] = desc, views, (host, names)
    return _BUILT[name]


def pack_op(desc, views, op, knobs=None, n_views=None):
    """(rc, dict of what tv_diag_pack_op reports) for one op; the buffers as bytes."""
    from tauv_vision_amd import _lib
    L = _lib.lib()
    info, label = (ctypes.c_int32 * 5)(), ctypes.create_string_buffer(256)
    segs, size = ((ctypes.c_int32 * 6) * 8)(), (ctypes.c_int64 * 3)()
    n = len(views) if n_views is None else n_views
    head = (ctypes.byref(desc), views, n, knobs, op, info, label, 256, segs, 8, size)
    rc = L.tv_diag_pack_op(*head, None, None, None, None)
    if rc:
        return rc, dict(n_ops=info[0])
    bufs = [ctypes.create_string_buffer(max(1, int(s))) for s in size]
    rc = L.tv_diag_pack_op(*head, *bufs, size)
    assert rc == 0
    return 0, dict(n_ops=info[0], kind=info[1], Npad=info[2], Kpad=info[3], label=label.value.decode(),
                   segs=[tuple(segs[i]) for i in range(info[4])], sizes=[int(s) for s in size],
                   weight=bufs[0].raw[:size[0]], bias=bufs[1].raw[:size[1]], extra=bufs[2].raw[:size[2]])


def packed_ops(name, precision):
    desc, views, _ = built(name)
    d = desc(precision)
    rc, first = pack_op(d, views, 0)
    assert rc == 0
    return [first] + [pack_op(d, views, i)[1] for i in range(1, first["n_ops"])]


def digests(ops):
    """(SHA-256 over every op's report in op order, 8 hex digits per op)."""
    total, short = hashlib.sha256(), []
    for o in ops:
        head = np.array([o["kind"], o["Npad"], o["Kpad"], len(o["segs"])] + [v for s in o["segs"] for v in s] +
                        o["sizes"], dtype=np.int64).tobytes()
        blob = o["label"].encode() + b"\0" + head + o["weight"] + o["bias"] + o["extra"]
        total.update(blob)
        short.append(hashlib.sha256(blob).hexdigest()[:8])
    return total.hexdigest(), "".join(short)


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_packed_bytes_are_pinned(name, precision):
    ops = packed_ops(name, precision)
    want = _fixture()[name][precision]
    sha, short = digests(ops)
    assert len(ops) == len(want["ops"]) // 8, "the plan's op count changed"
    moved = [f"op {i} ({o['label']})" for i, o in enumerate(ops)
             if short[8 * i:8 * i + 8] != want["ops"][8 * i:8 * i + 8]]
    assert not moved, f"{name} {precision}: packed bytes changed for {moved}"
    assert sha == want["sha256"]


def test_cases_reach_the_flavours_a_report_shows():
    """Of the flavours the cases were chosen for, those that show in a report: the depthwise
    ConvTranspose, ConvTranspose + skip, several K segments, convt3 fragments, fused-head fragments."""
    seen = set()
    for name in CASES:
        for o in packed_ops(name, "fp16"):
            seen.add({5: "depthwise convt", 2: "convt + skip"}.get(o["kind"], "multi-segment" if len(o["segs"]) > 1
                                                                  else "plain"))
            if o["extra"]:  # head fragments: per 128 hidden channels 8 KiB of fragments + 32 fp32, then 2 x 16 int32
                nts = o["segs"][0][2] // 128
                seen.add("head fragments" if len(o["extra"]) == nts * (8192 + 128) + 128 else "convt3 fragments")
    assert {"depthwise convt", "convt + skip", "multi-segment", "convt3 fragments", "head fragments"} <= seen


def _bn_of(label):
    for conv, bn in ((".conv1", ".bn1"), (".conv", ".bn"), (".0", ".1")):
        if label.endswith(conv):
            return label[:-len(conv)] + bn
    return None


@pytest.mark.parametrize("name", R18_CASES)
def test_plain_conv_ops_mean_the_folded_weight(name):
    """Every single-segment, unstacked, not row-expanded OP_CONV whose source stores exactly the
    weight's input channels, in fp32."""
    sd = {k: v.numpy() for k, v in case_state_dict(name).items()}
    covered = 0
    for o in packed_ops(name, "fp32"):
        w = sd.get(o["label"] + ".weight")
        if o["kind"] != OP_CONV or len(o["segs"]) != 1 or w is None:
            continue
        kh, kw, cs, ci0, cin, ks = o["segs"][0]
        n, wcin = w.shape[:2]
        if (kh, kw) != w.shape[2:] or cs != wcin or cin != wcin or ci0:  # (the row-expanded stem: cs = 24)
            continue
        bn = _bn_of(o["label"])
        b = sd.get(o["label"] + ".bias", np.zeros(n, np.float32)).astype(np.float64)
        scale, shift = np.ones(n), b
        has_bn = bn is not None and bn + ".running_mean" in sd
        if has_bn:
            g, beta, mean, var = (sd[f"{bn}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean",
                                                                                  "running_var"))
            scale = g / np.sqrt(var + 1e-5)
            shift = (b - mean) * scale + beta
        Npad, Kpad = o["Npad"], o["Kpad"]
        assert Kpad == 32 * ks and Npad % 128 == 0 and Npad >= n
        got = np.frombuffer(o["weight"], np.float32).reshape(Npad, Kpad)
        want = np.zeros((Npad, Kpad), np.float32)
        # [co][ci][t] -> [co][t * cs + ci]
        want[:n, :kh * kw * cs] = (w.astype(np.float64).reshape(n, wcin, kh * kw) * scale[:, None, None]) \
            .astype(np.float32).transpose(0, 2, 1).reshape(n, -1)
        np.testing.assert_array_equal(got, want, err_msg=o["label"])
        bias = np.frombuffer(o["bias"], np.float32)
        assert bias.shape == (Npad,) and not bias[n:].any()
        ref = shift.astype(np.float32)
        if has_bn:
            assert (np.abs(bias[:n] - ref) <= np.spacing(np.abs(ref))).all(), o["label"]
        else:
            np.testing.assert_array_equal(bias[:n], ref, err_msg=o["label"])
        covered += 1
    print(f"{name}: {covered} plain conv ops compared")
    assert covered > 0


def test_refusals():
    from tauv_vision_amd import _lib
    L = _lib.lib()
    desc, views, (host, names) = built("r18_c16_b2_96x128")
    d = desc("fp32")
    rc, rep = pack_op(d, views, 0)
    assert rc == 0
    for bad in (-1, rep["n_ops"]):
        assert pack_op(d, views, bad)[0] == _lib.TV_EINVAL
        assert "op index out of range" in L.tv_last_error().decode()
    # op 1 is the stem: its conv weight and its BatchNorm
    key = "backbone.dla_down.projection_layer.0.weight"
    i = list(host).index(key)
    keep = views[i].name, views[i].numel
    try:
        views[i].numel = keep[1] - 1
        assert pack_op(d, views, 1)[0] == _lib.TV_ENOTFOUND
        assert L.tv_last_error().decode() == f"state_dict key {key}: expected {keep[1]} elements, got {keep[1] - 1}"
        views[i].numel = keep[1]
        views[i].name = b"not.a.key"
        assert pack_op(d, views, 1)[0] == _lib.TV_ENOTFOUND
        assert L.tv_last_error().decode() == f"missing state_dict key: {key}"
    finally:
        views[i].name, views[i].numel = keep
    assert pack_op(d, views, 1)[0] == 0


def _regenerate():
    out = {}
    for name in CASES:
        out[name] = {}
        for p in PRECISIONS:
            sha, short = digests(packed_ops(name, p))
            out[name][p] = {"sha256": sha, "ops": short}
            print(name, p, len(short) // 8, "ops", sha[:16])
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_pack_cpu.py --regenerate")
    _regenerate()
