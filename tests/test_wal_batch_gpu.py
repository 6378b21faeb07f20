"""GPU side of the batch WAL commit: the fused ingest path on cuda:0 with
_wal_batch on against the same data with it off (live and after replay), and
the packed device call, which now queues its copy and launch with the GIL
released, at its smallest and at a ring-growing batch size."""

import threading

import pytest
import torch

from greptimedb_amd.engine.engine import EngineConfig, MitoEngine
from greptimedb_amd.engine.ingest import Ingestor
from greptimedb_amd.models.tsbs import CpuWorkload
from greptimedb_amd.query.executor import Executor

pytestmark = pytest.mark.gpu

_SQL = ("SELECT hostname, count(*), min(usage_user), max(usage_user), "
        "min(usage_idle), max(usage_idle) FROM cpu GROUP BY hostname "
        "ORDER BY hostname")


def _engine(path, device="cuda:0"):
    return MitoEngine(EngineConfig(data_dir=str(path), device=device,
                                   background_flush=False, wal_shards=4))


def _query(eng):
    r = Executor(eng).execute(_SQL)
    return [list(c) for c in r.columns]


def _worker_batches(tag, n=20, rows=300):
    w = CpuWorkload(scale=23, seed=31 + tag)
    w.tagsets = [t.replace(b"host_", b"host_%d_" % tag) for t in w.tagsets]
    return [w.next_batch(rows) for _ in range(n)]


def test_two_threads_batch_commit_matches_unbatched(tmp_path):
    data = [_worker_batches(0), _worker_batches(1)]
    results = {}
    for name, wal_batch in [("on", True), ("off", False)]:
        eng = _engine(tmp_path / name)
        fused, errors = [], []
        orig = eng.write_regions_fused
        eng.write_regions_fused = lambda *a, _o=orig, **kw: (fused.append(kw.get("wal_batch")), _o(*a, **kw))[1]

        def run(batches):
            try:
                ing = Ingestor(eng, default_regions=4, durable=True)
                ing._wal_batch = wal_batch
                assert ing._bulk and ing._fused and ing._packed
                for b in batches:
                    assert ing.ingest_lines(b) == 300
            except BaseException as e:   # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=run, args=(d,)) for d in data]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        # each worker's first batch registers its series on the general path
        assert fused == [wal_batch] * (2 * 19)
        assert len(eng.table("cpu").regions) == 4
        torch.cuda.synchronize()
        live = _query(eng)
        eng.close()
        eng = _engine(tmp_path / name)     # from WAL replay
        results[name] = (live, _query(eng))
        eng.close()
    live_on, replay_on = results["on"]
    live_off, replay_off = results["off"]
    assert len(live_on[0]) == 46 and sum(live_on[1]) == 2 * 20 * 300
    assert live_on == live_off
    assert replay_on == live_on and replay_off == live_on


def test_packed_call_smallest_and_ring_growing_batch(tmp_path):
    w = CpuWorkload(scale=10, seed=3)
    batches = [w.next_batch(50), w.next_batch(1), w.next_batch(3001),
               w.next_batch(1)]
    results = {}
    for name, device in [("cpu", "cpu"), ("gpu", "cuda:0")]:
        eng = _engine(tmp_path / name, device)
        ing = Ingestor(eng, default_regions=4)
        ing._bulk = True
        calls = []
        orig = eng.write_regions_fused
        eng.write_regions_fused = lambda *a, _o=orig, **kw: (calls.append(a[2]), _o(*a, **kw))[1]
        ring_bytes = []
        for b, rows in zip(batches, (50, 1, 3001, 1)):
            assert ing.ingest_lines(b) == rows
            ring_bytes.append(ing._ring[0].host.numel() if ing._ring else 0)
        assert calls == [1, 3001, 1]       # row counts of the fused batches
        assert ring_bytes[2] > ring_bytes[1] > 0    # 3001 rows grew the ring
        if device != "cpu":
            assert all(s.host.is_pinned() and s.dev.is_cuda for s in ing._ring)
            torch.cuda.synchronize()
        results[name] = _query(eng)
        eng.close()
    assert sum(results["cpu"][1]) == 50 + 1 + 3001 + 1
    assert results["gpu"] == results["cpu"]
