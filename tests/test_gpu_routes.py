"""The engine's route table: which kernel every op of every model runs, pinned for equality.

Routing is a function of the model's shapes, the precision, the batch and the device's CU count,
so the cases are the real models at real sizes; none runs a kernel (engine creation + prepare()
only). For each case the (op label, kernel instance name) list of every slice size of the batch
must equal tests/data/kernel_routes.json, recorded on an MI355X from the engine as it was before
the schedule was split into plan_schedule (schedule.cpp) and materialize: a selection pass that takes
or loses an op it should not shows here, whichever layer it is.

The fixture records the CU count it was made on; on a device with another count the grids, and
with them the routes, legitimately differ, and the test skips (the only skip).

Re-record (after a deliberate routing change): python tests/test_gpu_routes.py OUT.json
The file holds each model's label list and each distinct kernel name once, and a case as one line
of indices into them, cases in sorted order (_write_fixture; _fixture expands it again).
"""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":  # the recorder runs outside pytest: the import paths conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "tauv-vision_amd"), os.path.join(_root, "tests", "golden"),
               os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "kernel_routes.json")
R18 = "r18_c128_b1_480x640"
DLA = "b1_480x640_kp"


def _cases():
    """(id, family, model, precision, B, knobs)"""
    from helpers import models_index
    from recipe import case_by_name
    c = []
    for B in (1, 8, 9, 16, 64):  # 8 | 9: lat_group_max_b; 16, 64: two concurrent slices
        c.append(("centernet", R18, "fp16", B, {}))
    c.append(("centernet", R18, "bf16", 1, {}))
    c.append(("centernet", R18, "fp32", 1, {}))
    c.append(("centernet", R18, "fp32", 32, {}))
    c.append(("centernet", R18, "fp32x3", 1, {}))
    for k, v in (("TV_LATGROUP", 0), ("TV_BURST", 0), ("TV_BURST", 2), ("TV_HEADFUSE", 0), ("TV_STEMFUSE", 0),
                 ("TV_C1X1", 0)):
        c.append(("centernet", R18, "fp16", 1, {k: str(v)}))
    c.append(("centernet", R18, "fp16", 1, {"TV_CONV3": "0", "TV_CONV3S2": "0"}))
    c.append(("centernet", R18, "fp16", 8, {"TV_CUS": "64"}))
    for name in models_index():
        if name != R18:
            c.append(("centernet", name, "fp16", case_by_name(name)["batch"], {}))
    c.append(("dla34", DLA, "fp16", 1, {}))
    c.append(("dla34", DLA, "fp16", 32, {}))
    c.append(("dla34", DLA, "fp32", 1, {}))
    c.append(("dla34", DLA, "fp16", 1, {"TV_DCN_SPLIT": "0"}))
    c.append(("dla34", DLA, "fp16", 1, {"TV_DCN64": "0"}))
    c.append(("dla34", "b2_64x96", "fp16", 2, {}))
    c.append(("protonet", "protonet_f64_k16_b1_9x17", "fp16", 3, {}))
    c.append(("protonet", "protonet_f64_k16_b1_9x17", "fp16", 3, {"TV_CT3": "0"}))
    c.append(("protonet", "protonet_f256_k8_b1_45x80", "fp16", 1, {}))
    out = []
    for fam, name, prec, B, knobs in c:
        kid = ",".join(f"{k}={v}" for k, v in sorted(knobs.items()))
        out.append((f"{fam}:{name}:{prec}:B{B}" + (f":{kid}" if kid else ""), fam, name, prec, B, knobs))
    return out


def _engine(fam, name, precision):
    dev = torch.device("cuda", 0)
    if fam == "centernet":
        import test_gpu_forward as fwd
        model, _, _, case = fwd.build(name, precision)
        return model.engine(dev, case["in_h"], case["in_w"])
    if fam == "dla34":
        import test_gpu_dla34 as dla
        model, _, _, case = dla.build(name, precision)
        return model.engine(dev, case["in_h"], case["in_w"])
    from recipe import protonet_case, protonet_inputs
    from tauv_vision_amd.yolact import Masknet, YolactConfig
    c = protonet_case(name)
    sd, _ = protonet_inputs(c)
    m = Masknet(YolactConfig(640, 360, (24, 48, 96, 192, 384), (1,), (0.1, 0.2), feature_depth=c["F"],
                             n_prototype_masks=c["k"]), precision=precision)
    m.load_state_dict(sd)
    return m.cuda().engine(dev, c["H"], c["W"])


def routes(fam, name, precision, B, knobs):
    """{slice size: [[label, kernel], ...]} of a B-frame forward, without running one."""
    from tauv_vision_amd import _lib
    from tauv_vision_amd import engine as E
    prev = E._DIAG_KNOBS
    E._DIAG_KNOBS = dict(knobs)
    try:
        eng = _engine(fam, name, precision)
    finally:
        E._DIAG_KNOBS = prev
    eng.prepare(B)
    L = _lib.lib()
    out = {}
    for b in sorted(set(eng.slices(B))):
        n = 0
        while L.tv_engine_op_kernel(eng._h, b, n):  # "" past the last op
            n += 1
        labels = [L.tv_engine_op_label(eng._h, i).decode() for i in range(n)]
        out[str(b)] = [list(r) for r in zip(labels, eng.op_kernels(b, n))]
    return out


def _fixture():
    """{"cu_count", "cases": {id: {slice size: [[label, kernel], ...]}}} from the compact file: the label
    list of each model and every distinct kernel name are stored once, a case as indices into them."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    cases = {}
    for cid, c in fx["cases"].items():
        labels = fx["labels"][c["labels"]]
        cases[cid] = {b: [[labels[i], fx["kernels"][k]] for i, k in enumerate(ks)] for b, ks in c["kernels"].items()}
    return {"cu_count": fx["cu_count"], "cases": cases}


def _write_fixture(path, cu_count, cases):
    labels, kernels, out = [], [], {}
    for cid, c in sorted(cases.items()):  # by case id, so that a re-recording leaves unchanged routes' lines alone
        lab = [r[0] for r in next(iter(c.values()))]
        assert all([r[0] for r in rows] == lab for rows in c.values())
        if lab not in labels:
            labels.append(lab)
        for r in (r for rows in c.values() for r in rows):
            if r[1] not in kernels:
                kernels.append(r[1])
        out[cid] = {"labels": labels.index(lab), "kernels": {b: [kernels.index(r[1]) for r in rows] for b, rows in c.items()}}
    one = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:  # one line per case, per label list and per kernel name
        f.write('{"cu_count": %d,\n"labels": [\n%s\n],\n"kernels": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            cu_count, ",\n".join(one(v) for v in labels), ",\n".join(one(v) for v in kernels),
            ",\n".join(f"{one(cid)}: {one(c)}" for cid, c in out.items())))


@pytest.mark.parametrize("cid,fam,name,precision,B,knobs", _cases(), ids=[c[0] for c in _cases()])
def test_route_table(cid, fam, name, precision, B, knobs):
    fx = _fixture()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != fx["cu_count"]:
        pytest.skip(f"routes recorded on {fx['cu_count']} CUs, this device has {cus}")
    got = routes(fam, name, precision, B, knobs)
    want = fx["cases"][cid]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for b in want:
        assert len(got[b]) == len(want[b]) and len(got[b]) > 0, (b, len(got[b]), len(want[b]))
        diff = [(i, g, w) for i, (g, w) in enumerate(zip(got[b], want[b])) if g != w]
        assert not diff, f"{cid} slice of {b}: (op, got, recorded) {diff}"


if __name__ == "__main__":
    rec = {}
    for cid, fam, name, precision, B, knobs in _cases():
        rec[cid] = routes(fam, name, precision, B, knobs)
        print(cid, {b: len(r) for b, r in rec[cid].items()}, flush=True)
    _write_fixture(sys.argv[1], torch.cuda.get_device_properties(0).multi_processor_count, rec)
