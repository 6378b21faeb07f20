#!/usr/bin/env python
"""K20 cold tier: time ADMIN compress_table, and the first scan after it, on
a TSBS-shaped flushed table held in the region scan cache: 10 fields of
2-decimal clamped random walks, (series, ts)-sorted, with a sequence column.

  python scripts/bench_gorilla_encode.py [--scale 1000 --hours 8] [--host-path] [--off-grid]

One process = one measurement (fresh engine, cold allocator); prints one JSON
line. Uses only engine interfaces that predate the device encoder, so the
same file measures an older checkout; compare alternating runs and take
slowest-new against fastest-old. --host-path sets SstBatch._device_encode =
False where that switch exists.
"""

import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

Q_SCAN = "SELECT count(*) c, max(usage_user) m, min(usage_idle) s FROM cpu"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1000, help="hosts")
    ap.add_argument("--hours", type=int, default=8, help="360 points/host/h")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--host-path", action="store_true")
    ap.add_argument("--off-grid", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    import torch
    from greptimedb_amd.engine import sst as sst_mod
    from greptimedb_amd.engine.engine import EngineConfig, MitoEngine
    from greptimedb_amd.models.tsbs_fixture import load_cpu_fixture
    from greptimedb_amd.query.executor import Executor

    cuda = a.device.startswith("cuda")
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    if a.host_path:
        sst_mod.SstBatch._device_encode = False

    eng = MitoEngine(EngineConfig(data_dir=tempfile.mkdtemp(prefix="genc_"),
                                  device=a.device, background_flush=False))
    rows = load_cpu_fixture(eng, scale=a.scale, hours=a.hours)
    nf = 0
    for st in eng.tables.values():
        for r in st.regions:
            for b in r.sst_cache.values():
                # what a flush leaves: fixed-decimal metrics and a sequence.
                # Tensor / tensor is a true division; tensor / scalar may
                # multiply by the reciprocal, which lands off the grid
                # (--off-grid keeps that: the XOR-mode shape).
                cents = torch.round(b.fields * 100.0)
                b.fields = cents / 100.0 if a.off_grid else \
                    cents / torch.full_like(cents, 100.0)
                b.seq = torch.arange(b.n, dtype=torch.int64,
                                     device=b.ts.device)
                nf = b.fields.shape[0]
    ex = Executor(eng)
    hot = ex.execute(Q_SCAN).rows()          # warm kernels and the planner
    sync()

    t0 = time.perf_counter()
    r = ex.execute("ADMIN compress_table('cpu')")
    sync()
    t_compress = time.perf_counter() - t0
    bytes_before, bytes_after = int(r.columns[0][0]), int(r.columns[1][0])

    t0 = time.perf_counter()
    first = ex.execute(Q_SCAN).rows()
    sync()
    t_first = time.perf_counter() - t0

    t0 = time.perf_counter()
    again = ex.execute(Q_SCAN).rows()
    sync()
    t_hot = time.perf_counter() - t0
    assert first == hot == again, (hot, first, again)

    # the encoder alone: one field column (ts_bits = 0), device events
    kernel_gbps = None
    from greptimedb_amd import ops
    if cuda and hasattr(ops, "gorilla_encode"):
        b = next(b for st in eng.tables.values() for r in st.regions
                 for b in r.sst_cache.values())
        col = b.fields[0].contiguous()
        ops.gorilla_encode(b.ts, col, pack_ts=False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(10):
            ops.gorilla_encode(b.ts, col, pack_ts=False)
        ev[1].record()
        sync()
        kernel_gbps = round(col.numel() * 8 * 10 /
                            (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9, 1)

    in_bytes = rows * 8 * (nf + 2)            # ts + fields + seq read once
    print(json.dumps({
        "encode_column_GBps": kernel_gbps,
        "label": a.label, "device": a.device, "off_grid": a.off_grid,
        "rows": rows, "fields": nf,
        "device_encode": bool(getattr(sst_mod.SstBatch, "_device_encode",
                                      False)),
        "compress_s": round(t_compress, 4),
        "first_scan_s": round(t_first, 4),
        "hot_scan_s": round(t_hot, 4),
        "bytes_before": bytes_before, "bytes_after": bytes_after,
        "ratio": round(bytes_before / max(bytes_after, 1), 2),
        "encode_input_GBps": round(in_bytes / t_compress / 1e9, 2),
    }))
    eng.close()


if __name__ == "__main__":
    main()
