"""RecordGather with the angles section (gloo, world_size 2, CPU), in the pattern of test_sharding_cpu.py:
records, counts and angles of every rank travel in ONE collective and unpack to each rank's arrays in frame
order; without the option the packed layout is byte for byte what it was, and it is the prefix of the
layout with angles."""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tauv_vision_amd.decode import REC
from tauv_vision_amd.sharding import RecordGather, records_to_detections, shard_bounds
from test_sharding_cpu import K, frame_records, free_port


def frame_angles(f):
    """Deterministic stand-in for one frame's angles [K, 3]: NaN past the frame's count and for the pitch."""
    a = (f + np.arange(K * 3, dtype=np.float32).reshape(K, 3) * 0.125).astype(np.float32)
    a[:, 1] = np.nan
    a[f % (K + 1):] = np.nan
    return a


def worker(rank, world, port, n, q):
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        lo, hi = shard_bounds(n, rank, world)
        per = -(-n // world)
        rec = torch.zeros((per, K, REC))
        cnt = torch.zeros((per,), dtype=torch.int32)
        ang = torch.full((per, K, 3), float("nan"))
        for i, f in enumerate(range(lo, hi)):
            r, c = frame_records(f)
            rec[i], cnt[i], ang[i] = torch.from_numpy(r), c, torch.from_numpy(frame_angles(f))
        g = RecordGather(per, K, "cpu", angles=True)
        calls = []
        gather = dist.all_gather
        dist.all_gather = lambda *a, **k: (calls.append(1), gather(*a, **k))[1]
        try:
            buf = g(RecordGather.pack(rec, cnt, ang))
        finally:
            dist.all_gather = gather
        assert len(calls) == 1, "records, counts and angles travel in one collective"
        assert buf.shape == (world, (per * K * REC + per + per * K * 3) * 4)
        with pytest.raises(ValueError):
            g(RecordGather.pack(rec, cnt))  # the shorter buffer does not fit this gather
        all_rec, all_cnt, all_ang = g.unpack()
        if rank == 0:
            q.put((all_rec[:n].numpy().copy(), all_cnt[:n].numpy().copy(), all_ang[:n].numpy().copy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [8, 7])
def test_record_gather_with_angles_two_ranks(n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, n, q)) for r in range(2)]
    for p in procs:
        p.start()
    rec, cnt, ang = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ang.shape == (n, K, 3) and ang.dtype == np.float32
    for f in range(n):
        r, c = frame_records(f)
        assert np.array_equal(rec[f], r) and cnt[f] == c
        assert np.array_equal(ang[f], frame_angles(f), equal_nan=True)
    dets = records_to_detections(rec, cnt, True, ang)
    assert [len(d) for d in dets] == [f % (K + 1) for f in range(n)]
    d = dets[3][1]
    assert d.pitch is None and d.roll == float(frame_angles(3)[1, 0]) and d.yaw == float(frame_angles(3)[1, 2])


def test_layout_without_angles_is_unchanged_and_a_prefix():
    per = 3
    rec = torch.arange(per * K * REC, dtype=torch.float32).view(per, K, REC)
    cnt = torch.tensor([2, 0, 5], dtype=torch.int32)
    ang = torch.arange(per * K * 3, dtype=torch.float32).view(per, K, 3) + 0.5
    plain = RecordGather.pack(rec, cnt)
    # the layout of before: the records' bytes, then the counts' bytes
    want = np.concatenate([np.frombuffer(rec.numpy().tobytes(), np.uint8), np.frombuffer(cnt.numpy().tobytes(), np.uint8)])
    assert plain.dtype == torch.uint8 and np.array_equal(plain.numpy(), want)
    full = RecordGather.pack(rec, cnt, ang)
    assert full.numel() == plain.numel() + per * K * 3 * 4
    assert torch.equal(full[:plain.numel()], plain)
    assert np.array_equal(full[plain.numel():].numpy(), np.frombuffer(ang.numpy().tobytes(), np.uint8))
