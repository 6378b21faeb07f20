"""MitoEngine: tables → regions on one device, WAL, flush scheduling.

Reference parity: src/mito2/src/engine.rs + worker.rs (WorkerGroup /
RegionWorker event loops) + src/catalog. MI355X redesign: one engine
instance per GPU (one process per GPU under torch.distributed); regions of
a table are sharded across engines by the partition rule (parallel/
partition.py). Background flush runs on a worker thread; WAL commits group
all regions of a write batch (reference handle_write.rs:611 batched
write_wal).
"""

from __future__ import annotations

import json
import os
import queue
import threading
from dataclasses import dataclass, field

import numpy as np

from greptimedb_amd.engine.region import Region
from greptimedb_amd.engine.wal import Wal, decode_batch, encode_batch
from greptimedb_amd.models.schema import TableSchema, region_id as make_region_id
from greptimedb_amd.utils.errors import (InvalidArguments, TableAlreadyExists,
                                         TableNotFound)


@dataclass
class EngineConfig:
    data_dir: str = "./greptime_data"
    device: str = "cpu"
    flush_bytes: int = 512 << 20        # per-region memtable flush threshold
    wal_sync: bool = False              # fdatasync per commit
    wal_segment_bytes: int = 256 << 20
    wal_shards: int = 1                 # parallel WAL writers (P5 workers)
    default_regions: int = 4
    background_flush: bool = True
    scan_mem_bytes: int = 32 << 30      # host-side scan materialization quota
    record_events: bool = False         # persist DDL/migration events table
    gc_interval_s: float = 600.0        # background orphan-SST scan period
    gc_grace_s: float = 3600.0          # spare files younger than this
    cold_compress_s: float = 0.0        # Gorilla-pack SST batches idle this
                                        # long (0 = disabled; K20 cold tier)
    global_write_buffer_bytes: int = 16 << 30   # node-wide memtable cap
                                        # (reference WriteBufferManagerImpl)


MERGE_MODES = ("last_row", "last_non_null")


def check_merge_mode(schema, append_mode: bool, merge_mode: str) -> None:
    """Validate a table's merge_mode (reference: mito2 MergeMode region
    option; it rejects the append_mode combination the same way)."""
    if merge_mode not in MERGE_MODES:
        raise InvalidArguments(
            f"invalid merge_mode {merge_mode!r}: expected 'last_row' or "
            "'last_non_null'")
    if merge_mode != "last_non_null":
        return
    if append_mode:
        raise InvalidArguments(
            "merge_mode 'last_non_null' cannot be combined with "
            "append_mode 'true': append tables keep every row")
    if any(c.dtype.is_string_like and c.fulltext
           for c in schema.field_columns):
        raise InvalidArguments(
            "merge_mode 'last_non_null' is not supported on a table with a "
            "FULLTEXT column: merged scan sources cannot keep per-segment "
            "posting row numbers")


@dataclass
class TableState:
    schema: TableSchema
    regions: list = field(default_factory=list)
    append_mode: bool = False
    merge_mode: str = "last_row"   # or "last_non_null" (MERGE_MODES)
    rule: object = None   # cached PartitionRule (parallel/partition.py)
    # (copy of `regions`, the same in lock order, their ids): what the
    # fused write path needs per batch, rebuilt when `regions` changes
    fused_order: tuple = field(default=None, repr=False, compare=False)


class MitoEngine:
    def __init__(self, config: EngineConfig):
        self.config = config
        os.makedirs(config.data_dir, exist_ok=True)
        self.tables: dict[str, TableState] = {}
        self.next_table_id = 1024
        self._ddl_lock = threading.Lock()
        self._catalog_path = os.path.join(config.data_dir, "catalog.json")
        self.wal = Wal(os.path.join(config.data_dir, "wal"),
                       segment_bytes=config.wal_segment_bytes,
                       sync_on_commit=config.wal_sync,
                       shards=config.wal_shards)
        self._flush_q: queue.Queue = queue.Queue()
        self._flusher = None
        # observer seam (reference: mito2 engine/listener.rs WorkerListener —
        # used by the flow engine for dirty-window tracking and by tests for
        # deterministic background-task observation)
        self.write_listeners: list = []   # callback(table_name, min_ts, max_ts, n)
        self.flush_listeners: list = []   # callback(table_name, region_id)
        # insert mirroring (reference operator/src/insert.rs:1384
        # FlowMirrorTask): callbacks get the parsed columnar batch
        # callback(table_state, region, codes, ts_ms, fields, field_names)
        self.mirror_listeners: list = []
        from greptimedb_amd.utils.memquota import MemoryQuota
        self.scan_quota = MemoryQuota(config.scan_mem_bytes)
        self._load_catalog()
        self._replay_wal()
        if config.background_flush:
            self._flusher = threading.Thread(target=self._flush_loop, daemon=True)
            self._flusher.start()

    # ------------------------------------------------------------- catalog

    def _load_catalog(self):
        if not os.path.exists(self._catalog_path):
            return
        with open(self._catalog_path) as f:
            cat = json.load(f)
        self.next_table_id = cat["next_table_id"]
        self.views = dict(cat.get("views", {}))
        self.schemas = set(cat.get("schemas", []))
        for td in cat["tables"]:
            schema = TableSchema.from_dict(td["schema"])
            # catalogs written before merge_mode existed have no key
            merge_mode = td.get("merge_mode", "last_row")
            st = TableState(schema=schema, append_mode=td["append_mode"],
                            merge_mode=merge_mode)
            for rn in range(td["n_regions"]):
                rid = make_region_id(schema.table_id, rn)
                rdir = os.path.join(self.config.data_dir, "region", str(rid))
                st.regions.append(Region(rid, schema, rdir, device=self.config.device,
                                         append_mode=td["append_mode"],
                                         merge_mode=merge_mode))
            self.tables[schema.name] = st

    def _save_catalog(self):
        cat = {
            "next_table_id": self.next_table_id,
            "views": getattr(self, "views", {}),
            "schemas": sorted(getattr(self, "schemas", set())),
            "tables": [
                {
                    "schema": st.schema.to_dict(),
                    "n_regions": len(st.regions),
                    "append_mode": st.append_mode,
                    "merge_mode": st.merge_mode,
                }
                for st in self.tables.values()
            ],
        }
        tmp = self._catalog_path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(cat, f)
        os.rename(tmp, self._catalog_path)

    def create_table(self, schema: TableSchema, n_regions: int | None = None,
                     append_mode: bool = False, if_not_exists: bool = False,
                     merge_mode: str = "last_row") -> TableState:
        check_merge_mode(schema, append_mode, merge_mode)
        with self._ddl_lock:
            existed = schema.name in self.tables
            st = self._create_table_locked(schema, n_regions, append_mode,
                                           if_not_exists, merge_mode)
        if not existed and self.config.record_events:
            from greptimedb_amd.utils.events import EVENTS_TABLE, recorder_of
            if schema.name != EVENTS_TABLE:
                recorder_of(self).record("create_table", {
                    "table": schema.name, "regions": len(st.regions)})
        return st

    def _create_table_locked(self, schema, n_regions, append_mode,
                             if_not_exists, merge_mode="last_row") -> TableState:
        if schema.name in self.tables:
            if if_not_exists:
                return self.tables[schema.name]
            raise TableAlreadyExists(schema.name)
        if schema.table_id == 0:
            schema.table_id = self.next_table_id
        self.next_table_id = max(self.next_table_id, schema.table_id) + 1
        n_regions = n_regions or self.config.default_regions
        st = TableState(schema=schema, append_mode=append_mode,
                        merge_mode=merge_mode)
        for rn in range(n_regions):
            rid = make_region_id(schema.table_id, rn)
            rdir = os.path.join(self.config.data_dir, "region", str(rid))
            st.regions.append(Region(rid, schema, rdir, device=self.config.device,
                                     append_mode=append_mode,
                                     merge_mode=merge_mode))
        self.tables[schema.name] = st
        self._save_catalog()
        return st

    def drop_table(self, name: str):
        st = self.tables.pop(name, None)
        if st is None:
            raise TableNotFound(name)
        self._save_catalog()
        if self.config.record_events:
            from greptimedb_amd.utils.events import EVENTS_TABLE, recorder_of
            if name != EVENTS_TABLE:
                recorder_of(self).record("drop_table", {"table": name})

    def truncate_table(self, name: str):
        """TRUNCATE: drop every region's data, keep the table definition
        (reference: TruncateTable DDL procedure → region truncate)."""
        st = self.table(name)
        for region in st.regions:
            region.truncate()
        if self.config.record_events:
            from greptimedb_amd.utils.events import recorder_of
            recorder_of(self).record("truncate_table", {"table": name})

    def table(self, name: str) -> TableState:
        try:
            return self.tables[name]
        except KeyError:
            raise TableNotFound(name) from None

    def partition_rule(self, st: TableState):
        """Resolve (and cache) the table's partition rule — multi-dim when
        `PARTITION ON COLUMNS` was declared, hash(pk) % n otherwise
        (reference: src/partition/src/manager.rs route resolution)."""
        if st.rule is None or st.rule.n_regions != len(st.regions):
            from greptimedb_amd.parallel.partition import rule_for_table
            st.rule = rule_for_table(st.schema, len(st.regions))
        return st.rule

    def region_of_tags(self, st: TableState, tags: tuple) -> int:
        """Region index for one series' ordered tag values."""
        rule = self.partition_rule(st)
        return rule.region_of({c.name: v for c, v in
                               zip(st.schema.tag_columns, tags)})

    # ------------------------------------------------------------- writes

    def write_region(self, table: TableState, region_idx: int,
                     series_codes: np.ndarray, ts_ms: np.ndarray,
                     fields: np.ndarray, new_series: list[tuple[int, bytes]],
                     durable: bool = True,
                     str_fields: dict[str, list] | None = None) -> int:
        """WAL-append + memtable-append one region's slice of a write batch.
        Caller must call `commit_wal()` after all regions of the batch
        (group commit — durability boundary)."""
        region: Region = table.regions[region_idx]
        if not region.writable:
            from greptimedb_amd.utils.errors import RegionFenced
            raise RegionFenced(f"region {region.region_id} is downgraded")
        seq = 0
        if durable:
            payload = encode_batch(series_codes, ts_ms, fields,
                                   region.field_names, new_series, str_fields)
            seq = self.wal.append(region.region_id, payload)
        region.append(series_codes, ts_ms, fields, seq, str_fields)
        for cb in self.mirror_listeners:
            cb(table, region, series_codes, ts_ms, fields, region.field_names)
        if self.write_listeners and len(ts_ms):
            lo, hi = int(np.min(ts_ms)), int(np.max(ts_ms))
            for cb in self.write_listeners:
                cb(table.schema.name, lo, hi, len(ts_ms))
        return seq

    def write_regions_bulk(self, targets, series_codes: np.ndarray,
                           ts_ms: np.ndarray, fields: np.ndarray,
                           order: np.ndarray, starts: np.ndarray,
                           ends: np.ndarray, durable: bool = True) -> bool:
        """K16 fast path: one scatter_append kernel writes EVERY region's
        slice of a routed write batch, replacing the per-region
        write_region → narrow+copy_ chain (~6 torch dispatches per region).

        targets[k] = (TableState, region_idx) for segment order[starts[k]:
        ends[k]]; series_codes/ts_ms/fields[nf, n] are in ORIGINAL row order
        and all targets must share one field layout (single table — the
        caller checks). Returns False when a target needs the slow path
        (text columns keep host-side row lists)."""
        import torch
        from greptimedb_amd.ops import kernels as ops

        n = len(ts_ms)
        if n == 0:
            return True
        nf = fields.shape[0]
        regions: list[Region] = [st.regions[ri] for st, ri in targets]
        if any(r.text_cols or r.memtable.str_cols or not r.writable
               for r in regions):
            return False
        # WAL first (host-side; replay is region-keyed, so one entry per region)
        seqs = [0] * len(regions)
        if durable:
            for k, ((st, ri), s, e) in enumerate(zip(targets, starts, ends)):
                rows = order[s:e]
                region = regions[k]
                payload = encode_batch(series_codes[rows], ts_ms[rows],
                                       fields[:, rows], region.field_names, [])
                seqs[k] = self.wal.append(region.region_id, payload)
        # lock all regions in a stable global order (no deadlock vs flush or
        # a concurrent bulk writer), reserve rows, launch, update metadata
        ordered = sorted(regions, key=lambda r: r.region_id)
        for r in ordered:
            r.lock.acquire()
        try:
            seg_lens = (ends - starts).astype(np.int64)
            bases = np.empty(len(regions), dtype=np.int64)
            for k, region in enumerate(regions):
                mem = region.memtable
                if mem.nf < nf:
                    mem.add_fields(nf - mem.nf)
                need = mem.len + int(seg_lens[k])
                if need > mem.cap:
                    mem._grow(need)
                bases[k] = mem.len
            # dst offsets / dense region ids back in ORIGINAL row order
            within = np.arange(n, dtype=np.int64) - np.repeat(starts, seg_lens)
            dst_sorted = np.repeat(bases, seg_lens) + within
            dense_sorted = np.repeat(np.arange(len(regions), dtype=np.int32),
                                     seg_lens)
            dst_off = np.empty(n, dtype=np.int64)
            dst_off[order] = dst_sorted
            region_of = np.empty(n, dtype=np.int32)
            region_of[order] = dense_sorted
            dev = self.config.device
            ts_t = torch.from_numpy(np.ascontiguousarray(ts_ms)).to(dev)
            se_t = torch.from_numpy(
                np.ascontiguousarray(series_codes, dtype=np.int32)).to(dev)
            f_t = torch.from_numpy(np.ascontiguousarray(fields)).to(dev)
            ro_t = torch.from_numpy(region_of).to(dev)
            do_t = torch.from_numpy(dst_off).to(dev)
            ops.scatter_append(ts_t, se_t, f_t, ro_t, do_t,
                               [r.memtable.ts for r in regions],
                               [r.memtable.series for r in regions],
                               [r.memtable.fields for r in regions])
            # per-segment min/max on host (reduceat over the region-sorted view)
            ts_sorted = ts_ms[order]
            seg_min = np.minimum.reduceat(ts_sorted, starts)
            seg_max = np.maximum.reduceat(ts_sorted, starts)
            for k, region in enumerate(regions):
                mem = region.memtable
                mem.len = int(bases[k] + seg_lens[k])
                mn, mx = int(seg_min[k]), int(seg_max[k])
                mem.min_ts = mn if mem.min_ts is None else min(mem.min_ts, mn)
                mem.max_ts = mx if mem.max_ts is None else max(mem.max_ts, mx)
                region.last_seq = max(region.last_seq, seqs[k])
                region.row_seq += int(seg_lens[k])
        finally:
            for r in reversed(ordered):
                r.lock.release()
        if self.mirror_listeners:
            for k, ((st_k, _ri), s_, e_) in enumerate(zip(targets, starts, ends)):
                rows = order[s_:e_]
                if len(rows) == 0:
                    continue
                for cb in self.mirror_listeners:
                    cb(st_k, regions[k], series_codes[rows], ts_ms[rows],
                       fields[:, rows], st_k.regions[0].field_names)
        if self.write_listeners:
            lo, hi = int(np.min(ts_ms)), int(np.max(ts_ms))
            names = {st.schema.name for st, _ in targets}
            for name in names:
                for cb in self.write_listeners:
                    cb(name, lo, hi, n)
        return True

    def write_regions_bulk_pre(self, table: TableState, series_codes: np.ndarray,
                               ts_ms: np.ndarray, fields: np.ndarray,
                               region_of: np.ndarray, dst_off: np.ndarray,
                               counts: np.ndarray, mins: np.ndarray,
                               maxs: np.ndarray, payloads: list,
                               durable: bool = True) -> bool:
        """K16 fast path with the host side precomputed by
        _native.route_ingest: WAL payloads, per-row destination offsets and
        per-region counts/min/max arrive ready-made — python only reserves
        rows, launches the scatter kernel and updates metadata."""
        import torch
        from greptimedb_amd.ops import kernels as ops

        regions: list[Region] = table.regions
        if any(r.text_cols or r.memtable.str_cols or not r.writable
               for r in regions):
            return False
        n = len(ts_ms)
        nf = fields.shape[0]
        seqs = [0] * len(regions)
        if durable:
            for k, p in enumerate(payloads):
                if p is not None:
                    seqs[k] = self.wal.append(regions[k].region_id, p)
        ordered = sorted(regions, key=lambda r: r.region_id)
        for r in ordered:
            r.lock.acquire()
        try:
            bases = np.empty(len(regions), dtype=np.int64)
            for k, region in enumerate(regions):
                mem = region.memtable
                if mem.nf < nf:
                    mem.add_fields(nf - mem.nf)
                need = mem.len + int(counts[k])
                if need > mem.cap:
                    mem._grow(need)
                bases[k] = mem.len
            dst = dst_off + bases[region_of]
            dev = self.config.device
            ts_t = torch.from_numpy(np.ascontiguousarray(ts_ms)).to(dev)
            se_t = torch.from_numpy(
                np.ascontiguousarray(series_codes, dtype=np.int32)).to(dev)
            f_t = torch.from_numpy(np.ascontiguousarray(fields)).to(dev)
            ro_t = torch.from_numpy(
                np.ascontiguousarray(region_of, dtype=np.int32)).to(dev)
            do_t = torch.from_numpy(dst).to(dev)
            ops.scatter_append(ts_t, se_t, f_t, ro_t, do_t,
                               [r.memtable.ts for r in regions],
                               [r.memtable.series for r in regions],
                               [r.memtable.fields for r in regions])
            for k, region in enumerate(regions):
                m = int(counts[k])
                if m == 0:
                    continue
                mem = region.memtable
                mem.len = int(bases[k]) + m
                mn, mx = int(mins[k]), int(maxs[k])
                mem.min_ts = mn if mem.min_ts is None else min(mem.min_ts, mn)
                mem.max_ts = mx if mem.max_ts is None else max(mem.max_ts, mx)
                region.last_seq = max(region.last_seq, seqs[k])
                region.row_seq += m
        finally:
            for r in reversed(ordered):
                r.lock.release()
        if self.mirror_listeners and n:
            fnames = table.regions[0].field_names
            for k, region in enumerate(regions):
                if int(counts[k]) == 0:
                    continue
                rows = np.flatnonzero(region_of == k)
                for cb in self.mirror_listeners:
                    cb(table, region, series_codes[rows], ts_ms[rows],
                       fields[:, rows], fnames)
        if self.write_listeners and n:
            lo, hi = int(np.min(ts_ms)), int(np.max(ts_ms))
            for cb in self.write_listeners:
                cb(table.schema.name, lo, hi, n)
        return True

    def write_regions_fused(self, table: TableState, slot, n: int, nf: int,
                            counts, mins, maxs, payloads: list,
                            durable: bool = True,
                            wal_batch: bool = False) -> None:
        """K16 fast path fed by LineParser.ingest_batch: the routed batch
        sits in one packed block (`slot.host`, layout of
        ops.cpu_ref.packed_segments) next to ready WAL payloads and
        per-region counts/min/max. Python appends the WAL entries, reserves
        rows under the region locks and makes ONE device call.

        wal_batch: the entries are appended AND committed here by
        Wal.append_commit_many (one GIL-free native call; the caller does
        not call commit_wal for this batch). Off: one Wal.append per region,
        and the caller commits.

        slot.dev set: ops.scatter_append_packed — one non-blocking copy of
        the pinned block plus one kernel on the current stream (on a CPU
        engine the reference implementation reads the block in place); the
        slot's event is recorded behind the launch so the owner can wait
        before refilling the block. slot.dev None: the block is ordinary
        host memory and its segments go through today's scatter_append.
        The caller has checked that no region has text columns and that all
        are writable."""
        import torch
        from greptimedb_amd.ops import cpu_ref
        from greptimedb_amd.ops import kernels as ops

        regions: list[Region] = table.regions
        cached = table.fused_order
        # Region has no __eq__, so the list comparison is one identity test
        # per element in C; it also sees a region replaced in place
        # (migration), which the identity of the list would not
        if cached is None or cached[0] != regions:
            cached = table.fused_order = (
                list(regions),
                tuple(sorted(regions, key=lambda r: r.region_id)),
                tuple(r.region_id for r in regions))
        ordered = cached[1]
        counts, mins, maxs = (
            a.tolist() if hasattr(a, "tolist") else [int(v) for v in a]
            for a in (counts, mins, maxs))
        seqs = [0] * len(regions)
        if durable and wal_batch:
            # the whole batch's frames in one native call: written (and
            # synced with wal_sync) before the rows are reserved below
            live = [k for k, p in enumerate(payloads) if p is not None]
            rids = cached[2]
            got = self.wal.append_commit_many(
                [rids[k] for k in live], [payloads[k] for k in live])
            for k, seq in zip(live, got):
                seqs[k] = seq
        elif durable:
            for k, p in enumerate(payloads):
                if p is not None:
                    seqs[k] = self.wal.append(regions[k].region_id, p)
        for r in ordered:
            r.lock.acquire()
        try:
            bases = []
            for k, region in enumerate(regions):
                mem = region.memtable
                if mem.nf < nf:
                    mem.add_fields(nf - mem.nf)
                need = mem.len + counts[k]
                if need > mem.cap:
                    mem._grow(need)
                bases.append(mem.len)
            dst_ts = [r.memtable.ts for r in regions]
            dst_se = [r.memtable.series for r in regions]
            dst_f = [r.memtable.fields for r in regions]
            if slot.dev is not None:
                ops.scatter_append_packed(slot.host, slot.dev, n, nf, bases,
                                          dst_ts, dst_se, dst_f)
                if slot.event is not None:
                    slot.event.record()
            else:
                ts_h, f_h, do_h, se_h, ro_h = cpu_ref.packed_segments(
                    slot.host, n, nf)
                dev = self.config.device
                dst = do_h + torch.tensor(bases, dtype=torch.int64)[ro_h.long()]
                ops.scatter_append(ts_h.to(dev), se_h.to(dev), f_h.to(dev),
                                   ro_h.to(dev), dst.to(dev),
                                   dst_ts, dst_se, dst_f)
            for k, region in enumerate(regions):
                m = counts[k]
                if m == 0:
                    continue
                mem = region.memtable
                mem.len = bases[k] + m
                mn, mx = mins[k], maxs[k]
                mem.min_ts = mn if mem.min_ts is None else min(mem.min_ts, mn)
                mem.max_ts = mx if mem.max_ts is None else max(mem.max_ts, mx)
                region.last_seq = max(region.last_seq, seqs[k])
                region.row_seq += m
        finally:
            for r in reversed(ordered):
                r.lock.release()
        if (self.mirror_listeners or self.write_listeners) and n:
            ts_h, f_h, _do, se_h, ro_h = (
                t.numpy() for t in cpu_ref.packed_segments(slot.host, n, nf))
            if self.mirror_listeners:
                fnames = table.regions[0].field_names
                for k, region in enumerate(regions):
                    if counts[k] == 0:
                        continue
                    rows = np.flatnonzero(ro_h == k)
                    for cb in self.mirror_listeners:
                        cb(table, region, se_h[rows], ts_h[rows],
                           f_h[:, rows], fnames)
            if self.write_listeners:
                lo, hi = int(np.min(ts_h)), int(np.max(ts_h))
                for cb in self.write_listeners:
                    cb(table.schema.name, lo, hi, n)

    def commit_wal(self):
        self.wal.commit()

    def maybe_flush(self):
        total = 0
        for st in self.tables.values():
            for region in st.regions:
                total += region.memtable.bytes_used
                if region.should_flush(self.config.flush_bytes):
                    if self._flusher is not None:
                        self._flush_q.put(region)
                    else:
                        self._flush_region(region)
        # global write-buffer accounting (reference WriteBufferManagerImpl):
        # when the NODE-wide memtable total exceeds the cap, flush the
        # largest memtables until projected usage is back under it — keeps
        # many under-threshold regions from accumulating unbounded HBM
        if total > self.config.global_write_buffer_bytes:
            regions = sorted(
                (r for st in self.tables.values() for r in st.regions
                 if r.memtable.bytes_used > 0),
                key=lambda r: r.memtable.bytes_used, reverse=True)
            for r in regions:
                if total <= self.config.global_write_buffer_bytes:
                    break
                total -= r.memtable.bytes_used
                if self._flusher is not None:
                    self._flush_q.put(r)
                else:
                    self._flush_region(r)

    def flush_all(self, wait: bool = True):
        for st in self.tables.values():
            for region in st.regions:
                self._flush_region(region)

    def _flush_region(self, region: Region):
        region.flush()
        self._purge_wal()
        # TWCS compaction check (reference: compaction scheduler kicks after
        # flush, mito2 flush.rs → compaction/scheduler.rs)
        from greptimedb_amd.engine.compaction import Compactor
        Compactor().compact_region(region)

    def compact_all(self):
        from greptimedb_amd.engine.compaction import Compactor
        c = Compactor()
        for st in self.tables.values():
            for region in st.regions:
                c.compact_region(region)

    def _flush_loop(self):
        # flush worker doubles as the periodic GC scheduler (reference:
        # metasrv's gc ticker; here the one background thread owns both)
        import queue as _queue
        import time as _time
        next_gc = _time.monotonic() + self.config.gc_interval_s
        while True:
            try:
                region = self._flush_q.get(timeout=max(
                    0.05, next_gc - _time.monotonic()))
            except _queue.Empty:
                region = False   # timer tick, not shutdown
            if region is None:
                return
            if region is not False:
                try:
                    self._flush_region(region)
                except Exception:  # pragma: no cover
                    import traceback
                    traceback.print_exc()
            if _time.monotonic() >= next_gc:
                next_gc = _time.monotonic() + self.config.gc_interval_s
                try:
                    self.gc_orphan_ssts(self.config.gc_grace_s)
                    self.apply_ttl()
                    self.compress_cold()
                except Exception:  # pragma: no cover
                    import traceback
                    traceback.print_exc()

    def compress_cold(self, age_s: float | None = None) -> int:
        """Gorilla-pack device-resident SST batches not scanned for
        `age_s` seconds (K20 cold tier — ~4.6× capacity on HBM at
        ~900 GB/s decode when a scan touches them again). Returns the
        number of batches packed. The reference approximates this with
        its disk page cache; here the compressed copy stays in HBM."""
        import time as _time
        age_s = age_s if age_s is not None else self.config.cold_compress_s
        if age_s <= 0:
            return 0
        cutoff = _time.monotonic() - age_s
        packed = 0
        for st in self.tables.values():
            for r in st.regions:
                with r.lock:
                    batches = list(r.sst_cache.values())
                for b in batches:
                    if b.ts is not None and b.last_access < cutoff:
                        b.compress()
                        packed += 1
        return packed

    def apply_ttl(self, now_ms: int | None = None) -> int:
        """Drop SSTs past their table's ttl option (reference: mito2
        compaction expels files whose max_ts < now - ttl). Returns the
        number of files removed. File-granular like the reference — rows
        inside a partially-expired file age out when the file does."""
        import time as _time
        from greptimedb_amd.query.parser import parse_interval_text
        now_ms = now_ms if now_ms is not None else int(_time.time() * 1000)
        removed = 0
        for st in self.tables.values():
            ttl = st.schema.options.get("ttl")
            if not ttl:
                continue
            try:
                ttl_ms = parse_interval_text(str(ttl))
            except Exception:
                continue
            if ttl_ms <= 0:
                continue
            cutoff = now_ms - ttl_ms
            for r in st.regions:
                with r.lock:
                    dead = [fid for fid, meta in r.manifest.files.items()
                            if int(meta.get("max_ts", 1 << 62)) < cutoff]
                    if not dead:
                        continue
                    r.manifest.commit({"kind": "edit", "files_to_add": [],
                                       "files_to_remove": dead})
                    for fid in dead:
                        r.sst_cache.pop(fid, None)
                for fid in dead:
                    for ext in (".parquet", ".ftidx"):
                        p = os.path.join(r.dir, "sst", f"{fid}{ext}")
                        try:
                            os.unlink(p)
                        except OSError:
                            pass
                    removed += 1
        return removed

    def gc_orphan_ssts(self, grace_s: float = 3600.0) -> int:
        """Delete SST/sidecar files no region manifest references
        (reference src/mito2/src/gc.rs orphan scan; metasrv global GC).
        Files younger than `grace_s` are spared — they may belong to an
        in-flight flush whose manifest edit has not landed yet."""
        import time as _time
        removed = 0
        now = _time.time()
        for st in self.tables.values():
            for r in st.regions:
                sdir = os.path.join(r.dir, "sst")
                if not os.path.isdir(sdir):
                    continue
                with r.lock:
                    known = set(r.manifest.files)
                for fn in os.listdir(sdir):
                    if not (fn.endswith(".parquet") or fn.endswith(".ftidx")):
                        continue
                    fid = fn.rsplit(".", 1)[0]
                    if fid in known:
                        continue
                    p = os.path.join(sdir, fn)
                    try:
                        if now - os.path.getmtime(p) < grace_s:
                            continue
                        os.unlink(p)
                        removed += 1
                    except OSError:
                        pass
        return removed

    def _purge_wal(self):
        """Purge WAL segments below every region's replay point. A region
        only constrains purging while it has unflushed WAL entries
        (wal.region_last > flushed_seq) — idle or never-written regions no
        longer pin the whole log (the reference obsoletes per region)."""
        with self.wal._lock:
            region_last = dict(self.wal.region_last)
        floors = []
        max_seen = 0
        for st in self.tables.values():
            for r in st.regions:
                last = region_last.get(r.region_id, 0)
                max_seen = max(max_seen, last)
                if last > r.flushed_seq:
                    floors.append(r.flushed_seq)
        self.wal.purge_before(min(floors) if floors else max_seen + 1)

    # ------------------------------------------------------------- recovery

    def _replay_wal(self):
        """Re-apply WAL entries above each region's flushed seq (reference:
        region/opener.rs:483 replay_memtable)."""
        regions = {r.region_id: (st, i)
                   for st in self.tables.values()
                   for i, r in enumerate(st.regions)}
        for _seg, rid, seq, payload in self.wal.replay():
            hit = regions.get(rid)
            if hit is None:
                continue
            st, idx = hit
            region: Region = st.regions[idx]
            if seq <= region.flushed_seq:
                continue
            series, ts, fields, fnames, new_series, str_cols = decode_batch(payload)
            # series codes are stable via the region series log (loaded at
            # open); payload new_series is belt-and-braces for a lost log tail
            for _code, pk in new_series:
                region.series.add_encoded(pk)
            # field order may differ from region's if schema evolved; map names
            if fnames != region.field_names:
                # auto-added fields that never reached a flush only exist in
                # the WAL — recreate them before mapping (else data is lost)
                missing = [fn for fn in fnames
                           if fn not in region.field_names]
                if missing:
                    region.ensure_fields(missing)
                fmap = {fn: i for i, fn in enumerate(fnames)}
                out = np.full((len(region.field_names), fields.shape[1]), np.nan)
                for i, fn in enumerate(region.field_names):
                    if fn in fmap:
                        out[i] = fields[fmap[fn]]
                fields = out
            region.append(series, ts, fields, seq, str_cols or None)

    def close(self):
        if self._flusher is not None:
            self._flush_q.put(None)
            self._flusher.join(timeout=10)
            self._flusher = None
        self.wal.close()
