#!/usr/bin/env python3
"""Where a fused ingest batch spends its wall time, per section, with N
workers side by side (profiles/2026-10-21_batch_commit.md).

  python scripts/profile_batch_commit.py sections --workers 6 [--wal-batch 0|1]
      [--crc auto|table] [--root TREE]
    bench.py's ingest setup (cuda:0 when present, 4 regions, 4 WAL shards,
    background flush live, 3000-row batches, one Ingestor per thread) with the
    sections of a steady-state batch wrapped in wall-clock timers. Prints ms
    per batch per section, averaged over workers. A section's time with six
    workers minus its time with one worker is time spent waiting (for the
    GIL, a lock, or a core).

  python scripts/profile_batch_commit.py bench [--wal-batch 0|1]
      [--crc auto|table] [--root TREE] -- <bench.py arguments>
    Runs TREE/bench.py unchanged after flipping the switches, to put each
    part's share of the headline figure on record.

--root picks the source tree (default: the one this script is in), so the
same script measures a parent checkout. Switches a tree does not have are
ignored with a note.
"""

import argparse
import os
import runpy
import sys
import threading
import time


def _setup(root, wal_batch, crc):
    sys.path.insert(0, root)
    import torch  # noqa: F401  (loads libc10 before the extension)
    from greptimedb_amd import _native
    from greptimedb_amd.engine.ingest import Ingestor
    if wal_batch is not None:
        _patch_wal_batch(Ingestor, bool(wal_batch))
    if crc == "table":
        if hasattr(_native, "crc32_force_table"):
            _native.crc32_force_table(True)
        else:
            print("# note: this tree has no crc32_force_table (table CRC only)")


def _patch_wal_batch(Ingestor, on):
    """Ingestor sets `_wal_batch` per instance; force it after __init__."""
    orig = Ingestor.__init__

    def init(self, *a, **kw):
        orig(self, *a, **kw)
        if hasattr(self, "_wal_batch"):
            self._wal_batch = on
        elif on:
            print("# note: this tree has no _wal_batch switch")
    Ingestor.__init__ = init


class _Acc(threading.local):
    def __init__(self):
        self.t = {}


class _ParserProxy:
    """Times ingest_batch of a LineParser (a pybind object takes no
    instance attributes)."""

    def __init__(self, parser, timed):
        self._p = parser
        self.ingest_batch = timed("ingest_batch", parser.ingest_batch)

    def __getattr__(self, name):
        return getattr(self._p, name)


def sections(args):
    import torch
    from greptimedb_amd.engine.engine import EngineConfig, MitoEngine
    from greptimedb_amd.engine.ingest import Ingestor
    from greptimedb_amd.models.tsbs import CpuWorkload
    from greptimedb_amd.ops import kernels as ops
    import tempfile
    import shutil

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    base = tempfile.mkdtemp(prefix="gdb_prof_")
    eng = MitoEngine(EngineConfig(data_dir=base, device=dev,
                                  background_flush=True, wal_shards=4,
                                  flush_bytes=64 << 20))
    acc = _Acc()
    all_accs = []

    def timed(name, fn):
        def wrapped(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                d = acc.t
                d[name] = d.get(name, 0.0) + time.perf_counter() - t0
        return wrapped

    eng.write_regions_fused = timed("write_regions_fused", eng.write_regions_fused)
    eng.commit_wal = timed("commit_wal", eng.commit_wal)
    eng.maybe_flush = timed("maybe_flush", eng.maybe_flush)
    eng.wal.append = timed("wal.append (all regions)", eng.wal.append)
    if hasattr(eng.wal, "append_commit_many"):
        eng.wal.append_commit_many = timed("wal.append_commit_many",
                                           eng.wal.append_commit_many)
    ops.scatter_append_packed = timed("device call", ops.scatter_append_packed)

    workers = []
    for wi in range(args.workers):
        w = CpuWorkload(scale=100, seed=7 + wi)
        w.tagsets = [t.replace(b"host_", b"host_0_%d_" % wi) for t in w.tagsets]
        batches = [w.next_batch(3000) for _ in range(args.pool)]
        ing = Ingestor(eng, default_regions=4, append_mode=True, durable=True)
        if dev == "cpu":
            ing._bulk = True
        ing.parser = _ParserProxy(ing.parser, timed)
        ing.ingest_lines = timed("total ingest_lines", ing.ingest_lines)
        workers.append((ing, batches))

    def run(nb, record):
        def fn(ing, batches):
            acc.t = {}
            for k in range(nb):
                ing.ingest_lines(batches[k % len(batches)])
            if record:
                all_accs.append(acc.t)
        ths = [threading.Thread(target=fn, args=wk) for wk in workers]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if dev != "cpu":
            torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(args.warmup, False)
    wall = run(args.batches, True)
    names = ["ingest_batch", "write_regions_fused", "wal.append (all regions)",
             "wal.append_commit_many", "device call", "commit_wal",
             "maybe_flush", "total ingest_lines"]
    avg = {n: sum(a.get(n, 0.0) for a in all_accs) / len(all_accs) /
           args.batches * 1e3 for n in names}
    wal = avg["wal.append (all regions)"] + avg["wal.append_commit_many"]
    avg["region locks + bookkeeping (write_regions_fused - WAL - device)"] = \
        avg["write_regions_fused"] - wal - avg["device call"]
    avg["python glue (total - listed)"] = avg["total ingest_lines"] - (
        avg["ingest_batch"] + avg["write_regions_fused"] + avg["commit_wal"] +
        avg["maybe_flush"])
    rows = args.workers * args.batches * 3000
    print(f"# device={dev} workers={args.workers} batches/worker={args.batches} "
          f"wal_batch={args.wal_batch} crc={args.crc}")
    print(f"# wall {wall:.3f}s = {rows / wall:,.0f} rows/s, "
          f"{wall / args.batches * 1e3:.3f} ms per batch per worker")
    print("| section | ms per batch |")
    print("|---|---|")
    for n, v in avg.items():
        print(f"| {n} | {v:.3f} |")
    eng.close()
    shutil.rmtree(base, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sections", "bench"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    ap.add_argument("--workers", type=int, default=6)
    ap.add_argument("--batches", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--wal-batch", type=int, default=None, choices=[0, 1])
    ap.add_argument("--crc", default="auto", choices=["auto", "table"])
    args, rest = ap.parse_known_args()
    args.rest = [a for a in rest if a != "--"]
    root = os.path.abspath(args.root)
    _setup(root, args.wal_batch, args.crc)
    if args.mode == "sections":
        sections(args)
    else:
        sys.argv = [os.path.join(root, "bench.py")] + args.rest
        runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
