"""Query executor: SQL AST → GPU scan/aggregate over region shards.

Reference parity: src/query (DataFusion planner/executor + dist_plan
MergeScan) — redesigned for the MI355X node: a query runs in-process against
this rank's regions; the hot aggregate shape (time-bucket + tag group-by +
sum/min/max/avg/count, i.e. TSBS single/double-groupby, cpu-max-all,
high-cpu) is detected and lowered to the fused HIP kernel
ops.ts_bucket_agg (K1+K2+K5). Everything else goes through a vectorized
torch fallback path (gather → sort/dedup → aggregate/project), still fully
on-device. Cross-rank combine (reference MergeScanExec / commutativity
split, dist_plan) is handled by the DistContext hooks: partial aggregates
are RCCL all-reduced (sum/count: SUM, min: MIN, max: MAX) after group-key
unification.
"""

from __future__ import annotations

from dataclasses import dataclass, field as dfield

import numpy as np
import torch

from greptimedb_amd.engine.engine import MitoEngine, TableState
from greptimedb_amd.engine.merge import (last_row_index, sort_last_rows,
                                         sort_perm)
from greptimedb_amd.models.schema import (
    ColumnSchema, DataType, SemanticType, TableSchema,
)
from greptimedb_amd.query import ast
from greptimedb_amd.query.parser import parse_sql
from greptimedb_amd.utils.errors import (InvalidArguments, PlanQuery,
                                         TableAlreadyExists, TableNotFound)
from greptimedb_amd.utils.timeutil import parse_ts_ms, trunc_unit_ms
from greptimedb_amd.ops import filter_series_time, ts_bucket_agg
from greptimedb_amd.ops.cpu_ref import MOMENT_KINDS

AGG_FUNCS = {"count", "sum", "min", "max", "avg", "mean", "last_value",
             "first_value"}
BUCKET_FUNCS = {"date_trunc", "date_bin", "time_bucket"}
MAX_BUCKETS = 8_000_000


class QueryResult:
    def __init__(self, names: list[str], columns: list, kinds: list[str] | None = None):
        self.names = names
        self.columns = columns  # list of np arrays / lists, same length
        self.kinds = kinds or ["" for _ in names]  # "ts" marks epoch-ms columns

    def __len__(self):
        return len(self.columns[0]) if self.columns else 0

    def rows(self):
        if not self.columns:
            return []
        return list(zip(*[list(c) for c in self.columns]))

    def to_dict(self):
        return {n: list(c) for n, c in zip(self.names, self.columns)}


# ------------------------------------------------------------------ planning


@dataclass
class BucketSpec:
    bucket_ms: int
    origin: int | None = None  # None → align to bucket_ms grid


@dataclass
class AggCall:
    func: str           # count/sum/min/max/avg  (count with arg=None == count(*))
    arg: str | None     # field column name


@dataclass
class _DeviceQuantilePlan:
    """What _plan_device_quantile hands to _exec_device_quantile."""
    sel: "ast.Select"          # the statement as written
    sel2: "ast.Select"         # + hidden GROUP BY / ORDER BY projections
    plan: "SelectPlan"         # plan of sel2
    grid: tuple                # (ts_lo, ts_hi, origin, bucket_ms, n_buckets)
    group_keys: dict
    region_luts: list
    n_slots: int
    calls: list                # repr of each distinct percentile call
    field_of_call: list        # its field column
    p_of_sel: list             # its p
    n_group: int               # hidden GROUP BY projections
    order_desc: list           # DESC flag per hidden ORDER BY projection
    null_fields: list          # fields with a hidden count() projection
    m_calls: list = dfield(default_factory=list)   # repr of each moment call
    m_kinds: list = dfield(default_factory=list)   # its function name
    m_sel_of_call: list = dfield(default_factory=list)  # index into m_pairs
    m_pairs: list = dfield(default_factory=list)   # distinct (x, y) fields


@dataclass
class SelectPlan:
    table: TableState
    ts_lo: int | None
    ts_hi: int | None
    tag_conj: list            # [(tag_name, [values])]
    residual: ast.Expr | None
    bucket: BucketSpec | None
    bucket_expr: ast.Expr | None
    group_tags: list[str]
    aggs: list[AggCall]
    projections: list
    order_by: list
    having: ast.Expr | None
    limit: int | None
    offset: int | None


def _moment_null_marker(i: int) -> "ast.Func":
    """Hidden projection that carries the NULL mask of the i-th moment call
    of a device plan through _finalize_agg (no SQL function has this name)."""
    return ast.Func("__moment_null", [ast.Lit(i)])


def _split_conjuncts(e: ast.Expr) -> list[ast.Expr]:
    if isinstance(e, ast.BinOp) and e.op == "and":
        return _split_conjuncts(e.left) + _split_conjuncts(e.right)
    return [e]


def _lit_ts_ms(v, is_ts: bool):
    """Coerce a literal compared against the time index to epoch ms."""
    if isinstance(v, str):
        ms = parse_ts_ms(v)
        if ms is None:
            raise InvalidArguments(f"bad timestamp literal {v!r}")
        return ms
    return int(v)


def _expr_cols(e: ast.Expr) -> set:
    out = set()

    def walk(x):
        if isinstance(x, ast.Col):
            out.add(x.name)
        elif isinstance(x, ast.BinOp):
            walk(x.left); walk(x.right)
        elif isinstance(x, ast.UnaryOp):
            walk(x.operand)
        elif isinstance(x, ast.Cast):
            walk(x.expr)
        elif isinstance(x, ast.Func):
            for a in x.args:
                walk(a)
        elif isinstance(x, ast.WindowFunc):
            for a in x.args:
                walk(a)
            for a in x.partition_by:
                walk(a)
            for a, _d in x.order_by:
                walk(a)
        elif isinstance(x, ast.Case):
            if x.operand is not None:
                walk(x.operand)
            for w, r in x.whens:
                walk(w)
                walk(r)
            if x.default is not None:
                walk(x.default)
        elif isinstance(x, ast.InList):
            walk(x.expr)
            for a in x.items:
                walk(a)
        elif isinstance(x, ast.Between):
            walk(x.expr); walk(x.low); walk(x.high)
        elif isinstance(x, ast.IsNull):
            walk(x.expr)
    walk(e)
    return out


def _same_expr(a: ast.Expr, b: ast.Expr) -> bool:
    return repr(a) == repr(b)


class Executor:
    def __init__(self, engine: MitoEngine, dist=None):
        self.engine = engine
        self.dist = dist  # parallel.dist.DistContext or None
        self._virtual: dict = {}   # CTE scope: name -> QueryResult
        from greptimedb_amd.query.session import Session
        self.session = Session()

    # ---------------------------------------------------------- entrypoints

    SLOW_QUERY_MS = 1000.0

    def execute(self, sql: str) -> QueryResult:
        import time as _time
        from greptimedb_amd.utils.tracing import tracer
        stmt = parse_sql(sql)
        t0 = _time.perf_counter()
        # process registry (reference: catalog process_manager + KILL)
        plist = getattr(self.engine, "process_list", None)
        if plist is None:
            plist = self.engine.process_list = {}
        pid = getattr(self.engine, "_next_pid", 1)
        self.engine._next_pid = pid + 1
        entry = {"sql": sql, "start": t0, "elapsed_ms": 0.0,
                 "state": "running", "cancel": False}
        plist[pid] = entry
        self._proc_entry = entry
        try:
            with tracer.span("sql.execute", statement=sql[:200],
                             stmt_type=type(stmt).__name__):
                r = self.execute_stmt(stmt)
        finally:
            entry["elapsed_ms"] = (_time.perf_counter() - t0) * 1000
            plist.pop(pid, None)
            self._proc_entry = None
        dt = (_time.perf_counter() - t0) * 1000
        if dt >= self.SLOW_QUERY_MS:
            # slow-query log (reference: common/frontend slow query events)
            log = getattr(self.engine, "slow_queries", None)
            if log is None:
                from collections import deque
                log = self.engine.slow_queries = deque(maxlen=128)
            log.append({"sql": sql[:500], "ms": round(dt, 1)})
        return r

    def _eval_session_const(self, e):
        """Session/system functions MySQL+PG clients probe on connect
        (reference: session context functions in common/function)."""
        from greptimedb_amd import __version__
        if isinstance(e, ast.SysVar):
            name = e.name.lower().removeprefix("session.") \
                .removeprefix("global.")
            if name == "version":
                return f"8.4.2-greptimedb-amd-{__version__}"
            if name in ("time_zone", "timezone", "system_time_zone"):
                return self.session.timezone
            if name in ("autocommit", "sql_mode"):
                return {"autocommit": 1, "sql_mode": ""}[name]
            return self.session.vars.get(name, "")
        if isinstance(e, ast.Func) and not e.args:
            fn = e.name.lower()
            if fn == "version":
                return f"greptimedb-amd {__version__}"
            if fn in ("database", "current_schema", "schema"):
                return self.session.schema
            if fn in ("current_user", "user", "session_user"):
                return "greptime"
            if fn == "connection_id":
                return 1
        if isinstance(e, ast.Col) and e.name.lower() in (
                "current_timestamp", "current_date", "current_time"):
            import time as _time
            return int(_time.time() * 1000)
        return _eval_const(e)

    def _cancel_check(self):
        """Raise if this query's process entry was KILLed — polled inside
        per-region scan loops so long scans terminate promptly
        (reference: process manager cancellation tokens checked by the
        stream adapters)."""
        e = getattr(self, "_proc_entry", None)
        if e is not None and e.get("cancel"):
            from greptimedb_amd.utils.errors import QueryCancelled
            raise QueryCancelled("query killed")

    def execute_stmt(self, stmt) -> QueryResult:
        self._qualify_names(stmt)
        if isinstance(stmt, ast.Use):
            schemas = getattr(self.engine, "schemas", set()) | \
                {"public", "greptime_private", "information_schema"}
            if stmt.schema not in schemas:
                raise TableNotFound(f"database {stmt.schema}")
            self.session.schema = stmt.schema
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.Kill):
            plist = getattr(self.engine, "process_list", {})
            entry = plist.get(stmt.pid)
            if entry is None:
                raise InvalidArguments(f"no such query id {stmt.pid}")
            entry["cancel"] = True
            entry["state"] = "cancelled"
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.SetVar):
            self.session.set_var(stmt.name, stmt.value)
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.ShowVariables):
            base = {"time_zone": self.session.timezone,
                    "current_schema": self.session.schema}
            base.update(self.session.vars)
            items = sorted(base.items())
            if stmt.like:
                import fnmatch
                pat = stmt.like.replace("%", "*").replace("_", "?")
                items = [(k, v) for k, v in items if fnmatch.fnmatch(k, pat)]
            return QueryResult(["Variable_name", "Value"],
                               [[k for k, _ in items], [str(v) for _, v in items]])
        if isinstance(stmt, ast.CreateDatabase):
            schemas = getattr(self.engine, "schemas", None)
            if schemas is None:
                schemas = self.engine.schemas = set()
            if stmt.name in schemas and not stmt.if_not_exists:
                raise TableAlreadyExists(f"database {stmt.name}")
            schemas.add(stmt.name)
            self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.DropDatabase):
            schemas = getattr(self.engine, "schemas", set())
            if stmt.name not in schemas:
                if not stmt.if_exists:
                    raise TableNotFound(f"database {stmt.name}")
            else:
                schemas.discard(stmt.name)
                for t in [t for t in list(self.engine.tables)
                          if t.startswith(stmt.name + ".")]:
                    self.engine.drop_table(t)
                self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.Select):
            return self._exec_select(stmt)
        if isinstance(stmt, ast.SetOp):
            return self._exec_setop(stmt)
        if isinstance(stmt, ast.CreateView):
            return self._exec_create_view(stmt)
        if isinstance(stmt, ast.DropView):
            views = getattr(self.engine, "views", {})
            if stmt.name not in views:
                if not stmt.if_exists:
                    raise TableNotFound(stmt.name)
            else:
                views.pop(stmt.name, None)
                self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.CreateTable):
            return self._exec_create(stmt)
        if isinstance(stmt, ast.DropTable):
            try:
                self.engine.drop_table(stmt.name)
            except Exception:
                if not stmt.if_exists:
                    raise
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.TruncateTable):
            self.engine.truncate_table(stmt.name)
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.DeclareCursor):
            r = self.execute_stmt(stmt.select)
            self.session.cursors[stmt.name] = [r, 0]
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.FetchCursor):
            cur = self.session.cursors.get(stmt.name)
            if cur is None:
                raise InvalidArguments(f"no such cursor {stmt.name!r}")
            r, pos = cur
            rows = list(r.rows())[pos: pos + max(stmt.count, 0)]
            cur[1] = pos + len(rows)
            cols = [list(c) for c in zip(*rows)] if rows else \
                [[] for _ in r.names]
            return QueryResult(r.names, cols, r.kinds)
        if isinstance(stmt, ast.CloseCursor):
            if self.session.cursors.pop(stmt.name, None) is None:
                raise InvalidArguments(f"no such cursor {stmt.name!r}")
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.ShowTables):
            names = sorted(self.engine.tables)
            if stmt.like:
                import re as _re2
                pat = _re2.compile(
                    "^" + _re2.escape(stmt.like).replace("%", ".*")
                    .replace("_", ".") + "$")
                names = [n for n in names if pat.match(n)]
            if stmt.full:
                return QueryResult(["Tables", "Table_type"],
                                   [names, ["BASE TABLE"] * len(names)])
            return QueryResult(["Tables"], [names])
        if isinstance(stmt, ast.ShowDatabases):
            extra = sorted(getattr(self.engine, "schemas", set()))
            dbs = sorted({"greptime_private", "information_schema", "public",
                          *extra})
            if stmt.like:
                import re as _re2
                pat = _re2.compile(
                    "^" + _re2.escape(stmt.like).replace("%", ".*")
                    .replace("_", ".") + "$")
                dbs = [d for d in dbs if pat.match(d)]
            return QueryResult(["Database"], [dbs])
        if isinstance(stmt, ast.ShowTableStatus):
            names = sorted(self.engine.tables)
            if stmt.like:
                import re as _re2
                pat = _re2.compile(
                    "^" + _re2.escape(stmt.like).replace("%", ".*")
                    .replace("_", ".") + "$")
                names = [n for n in names if pat.match(n)]
            rows = [(n, "mito-hip",
                     sum(r.num_rows for r in self.engine.tables[n].regions))
                    for n in names]
            return QueryResult(["Name", "Engine", "Rows"],
                               [list(c) for c in zip(*rows)] if rows
                               else [[], [], []])
        if isinstance(stmt, ast.ShowCreateTable):
            return self._show_create_table(stmt.name)
        if isinstance(stmt, ast.ShowCreateView):
            views = getattr(self.engine, "views", {})
            if stmt.name not in views:
                raise TableNotFound(stmt.name)
            return QueryResult(
                ["View", "Create View"],
                [[stmt.name],
                 [f"CREATE VIEW {stmt.name} AS {views[stmt.name]}"]])
        if isinstance(stmt, ast.ShowCreateFlow):
            fe = self._flow_engine()
            f = fe.flows.get(stmt.name)
            if f is None:
                raise TableNotFound(f"flow {stmt.name}")
            return QueryResult(
                ["Flow", "Create Flow"],
                [[stmt.name],
                 [f"CREATE FLOW {stmt.name} SINK TO {f.sink} AS "
                  f"{f.select_sql}"]])
        if isinstance(stmt, ast.ShowIndex):
            st = self.engine.table(stmt.name)
            rows = []
            for pos, pk in enumerate(st.schema.primary_key):
                rows.append([stmt.name, "PRIMARY", pk, pos + 1,
                             "greptime-inverted-index-v1"])
            rows.append([stmt.name, "TIME INDEX",
                         st.schema.time_index.name, 1, "time-index"])
            for sn, ft in sorted(st.regions[0].text_cols.items()):
                rows.append([stmt.name, "FULLTEXT INDEX", sn, 1,
                             "greptime-fulltext-index-v1"])
            return QueryResult(
                ["table", "key_name", "column_name", "seq_in_index",
                 "index_type"],
                [list(c) for c in zip(*rows)] if rows else
                [[], [], [], [], []])
        if isinstance(stmt, ast.DescribeTable):
            st = self.engine.table(stmt.name)
            cols = st.schema.columns
            extra = [fn for fn in st.regions[0].field_names
                     if not st.schema.has_column(fn)]
            names = [c.name for c in cols] + extra
            types = [c.dtype.value for c in cols] + ["float64"] * len(extra)
            sem = [SemanticType(c.semantic).name for c in cols] + ["FIELD"] * len(extra)
            return QueryResult(["Column", "Type", "Semantic"], [names, types, sem])
        if isinstance(stmt, ast.InsertValues):
            return self._exec_insert(stmt)
        if isinstance(stmt, ast.Tql):
            return self._exec_tql(stmt)
        if isinstance(stmt, ast.Admin):
            return self._exec_admin(stmt)
        if isinstance(stmt, ast.CreateFlow):
            self._flow_engine().create_flow(stmt.name, stmt.sink, stmt.query_sql,
                                            stmt.if_not_exists,
                                            expire_after_s=stmt.expire_after_s)
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.DropFlow):
            self._flow_engine().drop_flow(stmt.name)
            return QueryResult(["status"], [["ok"]])
        if isinstance(stmt, ast.ShowFlows):
            fe = self._flow_engine()
            return QueryResult(["Flow", "Sink", "Query"],
                               [[f.name for f in fe.flows.values()],
                                [f.sink for f in fe.flows.values()],
                                [f.select_sql for f in fe.flows.values()]])
        if isinstance(stmt, ast.Explain):
            return self._exec_explain(stmt)
        if isinstance(stmt, ast.Copy):
            return self._exec_copy(stmt)
        if isinstance(stmt, ast.Delete):
            return self._exec_delete(stmt)
        if isinstance(stmt, ast.AlterTable):
            return self._exec_alter(stmt)
        raise PlanQuery(f"unsupported statement {type(stmt).__name__}")

    def _show_create_table(self, name: str) -> QueryResult:
        """Render the DDL (ref: query show_create_table.rs)."""
        st = self.engine.table(name)
        schema = st.schema
        sql_type = {
            "string": "STRING", "float64": "DOUBLE", "float32": "FLOAT",
            "int64": "BIGINT", "int32": "INT", "int16": "SMALLINT",
            "int8": "TINYINT", "uint64": "BIGINT UNSIGNED",
            "uint32": "INT UNSIGNED", "uint8": "TINYINT UNSIGNED",
            "bool": "BOOLEAN", "binary": "BINARY", "json": "JSON",
            "timestamp_ms": "TIMESTAMP(3)", "timestamp_s": "TIMESTAMP(0)",
            "timestamp_us": "TIMESTAMP(6)", "timestamp_ns": "TIMESTAMP(9)",
        }
        lines = []
        seen = set()
        for c in schema.columns:
            seen.add(c.name)
            t = f"VECTOR({c.vector_dim})" if c.dtype.value == "vector" else \
                sql_type.get(c.dtype.value, c.dtype.value.upper())
            opts = ""
            if c.semantic == SemanticType.TIMESTAMP:
                opts = " NOT NULL"
            if c.fulltext:
                opts += " FULLTEXT INDEX"
            lines.append(f'  "{c.name}" {t}{opts}')
        for fn in st.regions[0].field_names:
            if fn not in seen:
                lines.append(f'  "{fn}" DOUBLE')
        for sn in st.regions[0].str_field_names:
            if sn not in seen:
                ft = " FULLTEXT INDEX" if sn in st.regions[0].text_cols else ""
                lines.append(f'  "{sn}" STRING{ft}')
        lines.append(f'  TIME INDEX ("{schema.time_index.name}")')
        if schema.primary_key:
            pk = ", ".join(f'"{t}"' for t in schema.primary_key)
            lines.append(f"  PRIMARY KEY ({pk})")
        body = ",\n".join(lines)
        opts = [f"  regions = {len(st.regions)}"]
        if st.append_mode:
            opts.append("  append_mode = 'true'")
        if st.merge_mode == "last_non_null":
            opts.append("  merge_mode = 'last_non_null'")
        for k, v in sorted(schema.options.items()):
            if k not in ("partition_rule", "merge_mode"):
                opts.append(f"  {k} = '{v}'")
        part = ""
        if schema.options.get("partition_rule"):
            from greptimedb_amd.parallel.partition import MultiDimPartitionRule
            rule = MultiDimPartitionRule.from_json(schema.options["partition_rule"])
            part = rule.to_sql() + "\n"
        ddl = (f'CREATE TABLE IF NOT EXISTS "{name}" (\n{body}\n)\n'
               f"{part}ENGINE=mito\nWITH(\n" + ",\n".join(opts) + "\n)")
        return QueryResult(["Table", "Create Table"], [[name], [ddl]])

    def _exec_alter(self, a: ast.AlterTable) -> QueryResult:
        """ALTER TABLE ADD COLUMN / SET opts / UNSET opts / RENAME
        (reference: alter DDL procedure; tags are immutable — only fields
        can be added)."""
        st = self.engine.table(a.table)
        if a.action == "set_options":
            st.schema.options.update(a.options)
            self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        if a.action == "unset_options":
            for k in a.options:
                st.schema.options.pop(k, None)
            self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        if a.action == "rename":
            new = a.options["to"]
            if new in self.engine.tables:
                from greptimedb_amd.utils.errors import TableAlreadyExists
                raise TableAlreadyExists(new)
            self.engine.tables[new] = self.engine.tables.pop(a.table)
            st.schema.name = new
            self.engine._save_catalog()
            return QueryResult(["status"], [["ok"]])
        name, typ, opts = a.column
        tl = typ.lower()
        if tl in ("string", "varchar", "text", "json"):
            for r in st.regions:
                r.ensure_str_fields([name], fulltext=opts.get("fulltext", True))
        else:
            for r in st.regions:
                r.ensure_fields([name])
        return QueryResult(["status"], [["ok"]])

    def _exec_delete(self, d: ast.Delete) -> QueryResult:
        """DELETE FROM t [WHERE ...]: rewrite affected region data.

        The reference appends OpType::Delete tombstones resolved at
        read/compaction time; with device-resident data we rewrite the
        affected SSTs directly (flush first so the memtable is included) —
        durable immediately, no tombstone debt on the scan path."""
        sel = ast.Select([(ast.Star(), None)], d.table, where=d.where)
        plan = self._plan_select(sel)
        st = plan.table
        device = self.engine.config.device
        ts_lo = plan.ts_lo if plan.ts_lo is not None else -(1 << 62)
        ts_hi = plan.ts_hi if plan.ts_hi is not None else (1 << 62)
        deleted = 0
        from greptimedb_amd.engine import sst as sst_mod
        import os as _os
        for region in st.regions:
            region.flush()
            cand = self._candidate_codes(region, plan)
            lut = None
            if cand is not None:
                lut = np.full(len(region.series), -1, dtype=np.int32)
                lut[np.asarray(cand, dtype=np.int64)] = 1
            lut_t = torch.as_tensor(lut, device=device) if lut is not None else None
            for fid in list(region.sst_cache.keys()):
                b = region.sst_cache[fid]
                from greptimedb_amd.engine.region import ScanSource
                src = ScanSource(b.ts, b.series, b.fields, b.n,
                                 {fn: i for i, fn in enumerate(b.field_names)},
                                 True, getattr(b, "str_cols", {}), None)
                del_mask = filter_series_time(b.ts, b.series, lut_t, ts_lo, ts_hi)
                if plan.residual is not None:
                    del_mask &= self._eval_mask(plan.residual, src, region, device)
                ndel = int(del_mask.sum())
                if ndel == 0:
                    continue
                deleted += ndel
                keep = (~del_mask).nonzero(as_tuple=True)[0]
                ts_t = b.ts[keep].contiguous()
                se_t = b.series[keep].contiguous()
                f_t = b.fields[:, keep].contiguous()
                keep_h = keep.cpu().numpy()
                new_strs = {sn: np.asarray(col, dtype=object)[keep_h]
                            for sn, col in getattr(b, "str_cols", {}).items()}
                new_fid = sst_mod.new_file_id()
                path = _os.path.join(region.dir, "sst", f"{new_fid}.parquet")
                meta = sst_mod.write_sst(
                    path, region.schema, region.series.pks,
                    se_t.cpu().numpy(), ts_t.cpu().numpy(), f_t.cpu().numpy(),
                    np.arange(ts_t.numel(), dtype=np.int64), b.field_names,
                    str_cols=new_strs)
                region.manifest.commit({
                    "kind": "edit", "files_to_add": [meta.to_dict()],
                    "files_to_remove": [fid]})
                nb = sst_mod.SstBatch(ts_t, se_t, f_t, None, meta.min_ts,
                                      meta.max_ts, b.field_names)
                nb.str_cols = new_strs
                for sn, arr in new_strs.items():
                    ft = region.text_cols.get(sn)
                    if ft is not None:
                        nb.text_index[sn] = ft.build_segment(list(arr), device)
                with region.lock:
                    region.sst_cache.pop(fid, None)
                    region.sst_cache[new_fid] = nb
                old = _os.path.join(region.dir, "sst", f"{fid}.parquet")
                if _os.path.exists(old):
                    _os.unlink(old)
        return QueryResult(["rows"], [[deleted]])

    @staticmethod
    def _copy_object_store(path: str, options: dict):
        """Resolve an `s3://bucket/key` COPY path to (store, key).
        Endpoint comes from the WITH/CONNECTION `endpoint` option or
        GDB_S3_ENDPOINT (reference: common/datasource object-store URLs
        with CONNECTION (endpoint=..., access_key_id=...))."""
        if not path.startswith("s3://"):
            return None, path
        import os as _os
        from greptimedb_amd.engine.remote import S3ObjectStore
        rest = path[5:]
        bucket, _, key = rest.partition("/")
        endpoint = options.get("endpoint") or _os.environ.get("GDB_S3_ENDPOINT")
        if not endpoint:
            raise ValueError(
                "COPY s3:// needs an endpoint: WITH (endpoint='http://...') "
                "or GDB_S3_ENDPOINT")
        return S3ObjectStore(endpoint, bucket), key

    def _exec_copy(self, c: ast.Copy) -> QueryResult:
        """COPY table TO/FROM file or s3:// object (reference: operator COPY
        via common/datasource — parquet/csv/json by extension or WITH
        format; object-store targets staged through a temp file)."""
        import pyarrow as pa
        store, _key = self._copy_object_store(c.path, c.options)
        if store is not None:
            import tempfile as _tf
            import os as _os
            suffix = _os.path.splitext(_key)[1] or ".parquet"
            tmp = _tf.NamedTemporaryFile(suffix=suffix, delete=False)
            tmp.close()
            try:
                sub = ast.Copy(direction=c.direction, table=c.table,
                               path=tmp.name, options=dict(c.options))
                if c.direction == "from":
                    with open(tmp.name, "wb") as f:
                        f.write(store.get(_key))
                res = self._exec_copy(sub)
                if c.direction == "to":
                    with open(tmp.name, "rb") as f:
                        store.put(_key, f.read())
                return res
            finally:
                _os.unlink(tmp.name)
        fmt = c.options.get("format")
        if fmt is None:
            fmt = ("parquet" if c.path.endswith(".parquet")
                   else "csv" if c.path.endswith(".csv")
                   else "json" if c.path.endswith(".json") else "parquet")
        if c.direction == "to":
            r = self.execute_stmt(ast.Select([(ast.Star(), None)], c.table))
            arrays, names = [], []
            for n2, col, kind in zip(r.names, r.columns, r.kinds):
                names.append(n2)
                if kind == "ts":
                    arrays.append(pa.array(np.asarray(col, dtype=np.int64),
                                           type=pa.timestamp("ms")))
                else:
                    try:
                        arrays.append(pa.array(np.asarray(col, dtype=np.float64)))
                    except (ValueError, TypeError):
                        arrays.append(pa.array([None if v is None else str(v)
                                                for v in col], type=pa.string()))
            t = pa.Table.from_arrays(arrays, names=names)
            if fmt == "parquet":
                import pyarrow.parquet as pq
                pq.write_table(t, c.path)
            elif fmt == "csv":
                import pyarrow.csv as pacsv
                pacsv.write_csv(t, c.path)
            else:
                with open(c.path, "w") as f:
                    import json as _json
                    for row in r.rows():
                        f.write(_json.dumps(dict(zip(r.names, [
                            v if not isinstance(v, (np.generic,)) else v.item()
                            for v in row]))) + "\n")
            return QueryResult(["rows"], [[len(r)]])
        # COPY FROM
        if fmt == "parquet":
            import pyarrow.parquet as pq
            t = pq.read_table(c.path)
        elif fmt == "csv":
            import pyarrow.csv as pacsv
            t = pacsv.read_csv(c.path)
        else:
            import json as _json
            rows = [_json.loads(l) for l in open(c.path) if l.strip()]
            cols = {k: [r.get(k) for r in rows] for k in (rows[0] if rows else {})}
            t = pa.Table.from_pydict(cols)
        st = self.engine.table(c.table)
        schema = st.schema
        ts_name = schema.time_index.name
        tag_names = [cc.name for cc in schema.tag_columns]
        data = {cn: t.column(cn).to_pylist() for cn in t.column_names}
        n = t.num_rows
        ts_col = t.column(ts_name)
        if pa.types.is_timestamp(ts_col.type):
            ts_ms = ts_col.cast(pa.int64()).to_numpy(zero_copy_only=False)
            unit = ts_col.type.unit
            ts_ms = ts_ms // {"s": 1, "ms": 1, "us": 1000, "ns": 1_000_000}.get(unit, 1)
            if unit == "s":
                ts_ms = ts_ms * 1000
        else:
            ts_ms = np.asarray(data[ts_name], dtype=np.int64)
        field_names = st.regions[0].field_names
        str_names = st.regions[0].str_field_names
        from greptimedb_amd.engine import pk_codec
        from greptimedb_amd.engine.series import tsid_hash
        rows_by_region: dict[int, list[int]] = {}
        codes = np.empty(n, dtype=np.int32)
        for i in range(n):
            tags = tuple(None if data[tn][i] is None else str(data[tn][i])
                         for tn in tag_names)
            ridx = self.engine.region_of_tags(st, tags)
            codes[i] = st.regions[ridx].register_series(tags)
            rows_by_region.setdefault(ridx, []).append(i)
        for ridx, rows in rows_by_region.items():
            ra = np.array(rows)
            fmat = np.full((len(field_names), len(ra)), np.nan)
            for j, fn in enumerate(field_names):
                if fn in data:
                    col = np.asarray([data[fn][i] if data[fn][i] is not None
                                      else np.nan for i in ra], dtype=np.float64)
                    fmat[j] = col
            strs = {sn: [data[sn][i] for i in ra] for sn in str_names if sn in data}
            self.engine.write_region(st, ridx, codes[ra], ts_ms[ra], fmat, [],
                                     str_fields=strs or None)
        self.engine.commit_wal()
        return QueryResult(["rows"], [[n]])

    def _flow_engine(self):
        """Flow engine shared per storage engine (lazy)."""
        fe = getattr(self.engine, "flow_engine", None)
        if fe is None:
            from greptimedb_amd.flow.engine import FlowEngine
            fe = FlowEngine(self.engine, self)
            self.engine.flow_engine = fe
        return fe

    def _exec_admin(self, a: ast.Admin) -> QueryResult:
        """ADMIN functions (reference: common/function/src/admin/)."""
        f = a.func.lower()
        if f == "flush_table":
            st = self.engine.table(str(a.args[0]))
            for r in st.regions:
                self.engine._flush_region(r)
            return QueryResult(["result"], [[1]])
        if f == "compact_table":
            from greptimedb_amd.engine.compaction import Compactor
            st = self.engine.table(str(a.args[0]))
            c = Compactor(trigger_file_num=2)
            n = sum(c.compact_region(r) for r in st.regions)
            return QueryResult(["result"], [[n]])
        if f == "flow_tick":
            out = self._flow_engine().tick()
            return QueryResult(["flow", "rows"],
                               [list(out.keys()), list(out.values())])
        if f == "apply_ttl":
            return QueryResult(["files_removed"], [[self.engine.apply_ttl()]])
        if f == "compress_table":
            # K20 cold tier: pack resident SST batches into Gorilla blocks
            st = self.engine.table(str(a.args[0]))
            before = after = 0
            for r in st.regions:
                with r.lock:
                    for b in r.sst_cache.values():
                        if b.ts is not None:
                            before += b.n * (8 + 4 + 8 * b.fields.shape[0])
                            after += b.compress() + b.n * 4
            return QueryResult(["bytes_before", "bytes_after"],
                               [[before], [after]])
        if f == "gc":
            # orphan SST scan (reference src/mito2/src/gc.rs + metasrv gc.rs)
            grace = float(a.args[0]) if a.args else 3600.0
            n = self.engine.gc_orphan_ssts(grace_s=grace)
            return QueryResult(["result"], [[n]])
        if f == "flush_all":
            self.engine.flush_all()
            return QueryResult(["result"], [[1]])
        if f == "repartition_table":
            from greptimedb_amd.engine.repartition import repartition_table
            moved = repartition_table(self.engine, str(a.args[0]), int(a.args[1]))
            return QueryResult(["result"], [[moved]])
        if f == "migrate_region":
            from greptimedb_amd.meta.migration import migrate_region
            migrate_region(self.engine, str(a.args[0]), int(a.args[1]),
                           str(a.args[2]))
            return QueryResult(["result"], [[1]])
        if f == "build_vector_index":
            # ADMIN build_vector_index(table, col[, nlist[, nprobe]]) —
            # IVF-flat per SST source (ref: vector index per SST file)
            import math
            from greptimedb_amd.vector import build_ivf
            table, col = str(a.args[0]), str(a.args[1])
            nlist_arg = int(a.args[2]) if len(a.args) > 2 else 0
            nprobe = int(a.args[3]) if len(a.args) > 3 else 16
            st = self.engine.table(table)
            device = self.engine.config.device
            built = 0
            for region in st.regions:
                for b in region.sst_cache.values():
                    colv = b.str_cols.get(col)
                    if colv is None or not len(colv):
                        continue
                    vt = getattr(b, f"_vec_{col}", None)
                    if vt is None:
                        blob = b"".join(v if v is not None else b"" for v in colv)
                        flat = np.frombuffer(blob, dtype=np.float32)
                        lens = np.array([0 if v is None else len(v) // 4
                                         for v in colv])
                        D = int(lens.max()) if len(lens) else 0
                        if D == 0:
                            continue
                        full = np.full((len(colv), D), np.nan, dtype=np.float32)
                        full[lens > 0] = flat.reshape(-1, D)
                        vt = torch.as_tensor(full).to(device)
                        setattr(b, f"_vec_{col}", vt)
                    nlist = nlist_arg or max(8, int(4 * math.sqrt(vt.shape[0])))
                    setattr(b, f"_ivf_{col}", build_ivf(vt, nlist))
                    built += 1
                vi = getattr(region, "vector_index", None)
                if vi is None:
                    vi = region.vector_index = {}
                vi[col] = {"nlist": nlist_arg, "nprobe": nprobe}
            return QueryResult(["result"], [[built]])
        if f == "enable_tracing":
            from greptimedb_amd.utils.tracing import tracer
            tracer.enabled = bool(int(a.args[0])) if a.args else True
            if not tracer.enabled:
                tracer.drop()
            return QueryResult(["result"], [[int(tracer.enabled)]])
        if f == "flush_tracing":
            # export buffered internal spans into our own trace table via
            # the OTLP path (self-hosted observability)
            from greptimedb_amd.engine.tracestore import TraceStore
            from greptimedb_amd.utils.tracing import tracer
            ts_store = getattr(self.engine, "_internal_tracestore", None)
            if ts_store is None:
                ts_store = TraceStore(self.engine)
                self.engine._internal_tracestore = ts_store
            n = tracer.export_to(ts_store)
            return QueryResult(["result"], [[n]])
        raise PlanQuery(f"unknown admin function {a.func}")

    def _exec_explain(self, e: ast.Explain) -> QueryResult:
        """EXPLAIN [ANALYZE]: plan summary (+ execution metrics)."""
        import time as _time
        if not isinstance(e.stmt, ast.Select):
            raise PlanQuery("EXPLAIN supports SELECT")
        dq = self._plan_device_quantile(e.stmt)
        try:
            plan = dq.plan if dq is not None else self._plan_select(e.stmt)
        except PlanQuery as pq:
            # general-shape fallback (expression aggregates, GROUP BY on
            # fields, ORDER BY expressions): materialize + derived eval
            lines = ["Plan: materialize-fallback (derived-table eval)",
                     f"  reason: {pq}",
                     f"  table: {e.stmt.table}"]
            if e.analyze:
                t0 = _time.perf_counter()
                r = self.execute_stmt(e.stmt)
                lines.append(f"Execution: {len(r)} rows in "
                             f"{(_time.perf_counter() - t0) * 1000:.3f} ms")
            return QueryResult(["plan"], [lines])
        lines = []
        if dq is not None and not dq.calls:
            path = (f"grouped-moments (two-pass, M={len(dq.m_pairs)}, "
                    f"cells={dq.n_slots * dq.grid[4]})")
        elif dq is not None:
            moments = f", moments M={len(dq.m_pairs)}" if dq.m_pairs else ""
            path = (f"grouped-quantile (radix select, Q={len(dq.p_of_sel)}, "
                    f"cells={dq.n_slots * dq.grid[4]}{moments})")
        elif any(_has_range_agg(x) for x, _a in e.stmt.projections):
            path = "range-select (sliding-window kernel)"
        elif any(_collect_window_nodes(x, w := []) or w
                 for x, _a in e.stmt.projections):
            path = "raw-scan + window-functions"
        elif plan.aggs and plan.residual is None:
            path = "fused-ts-bucket-agg"
        elif plan.aggs:
            path = "agg-with-residual"
        else:
            path = "raw-scan"
        lines.append(f"Plan: {path}")
        if e.stmt.align_ms:
            lines.append(f"  align_ms: {e.stmt.align_ms} by: {e.stmt.align_by}")
        lines.append(f"  table: {plan.table.schema.name} "
                     f"regions={len(plan.table.regions)} append={plan.table.append_mode}")
        lines.append(f"  time_range: [{plan.ts_lo}, {plan.ts_hi})")
        lines.append(f"  tag_filters: {plan.tag_conj}")
        lines.append(f"  residual: {plan.residual}")
        if plan.bucket:
            lines.append(f"  bucket_ms: {plan.bucket.bucket_ms}")
        lines.append(f"  group_tags: {plan.group_tags}")
        lines.append(f"  aggs: {[(a.func, a.arg) for a in plan.aggs]}")
        if e.analyze:
            t0 = _time.perf_counter()
            r = self.execute_stmt(e.stmt)
            dt = (_time.perf_counter() - t0) * 1000
            lines.append(f"Execution: {dt:.3f} ms, {len(r)} output rows")
            srcs = sum(len(region.scan_sources(plan.ts_lo, plan.ts_hi))
                       for region in plan.table.regions)
            lines.append(f"  scan sources: {srcs}")
        return QueryResult(["plan"], [lines])

    def _exec_tql(self, t: ast.Tql) -> QueryResult:
        """TQL EVAL (start, end, step) expr — PromQL through SQL (reference:
        src/query/src/promql + sql TQL statement)."""
        from greptimedb_amd.query.promql.eval import PromEvaluator
        ev = PromEvaluator(self.engine, dist=self.dist)
        m = ev.query_range(t.query, t.start, t.end, t.step)
        label_keys = sorted({k for l in m.labels for k in l if k != "__name__"})
        ts_col, val_col = [], []
        label_cols = {k: [] for k in label_keys}
        vals = m.values.cpu().numpy()
        for s, labels in enumerate(m.labels):
            for ti, g in enumerate(m.grid):
                v = vals[s, ti]
                if np.isnan(v):
                    continue
                ts_col.append(int(g))
                val_col.append(float(v))
                for k in label_keys:
                    label_cols[k].append(labels.get(k))
        names = ["ts"] + label_keys + ["value"]
        cols = [np.asarray(ts_col)] + [np.asarray(label_cols[k], dtype=object)
                                       for k in label_keys] + [np.asarray(val_col)]
        return QueryResult(names, cols, ["ts"] + [""] * (len(names) - 1))

    # ---------------------------------------------------------- DDL / DML

    def _exec_create(self, c: ast.CreateTable) -> QueryResult:
        if c.external:
            return self._exec_create_external(c)
        type_map = {
            "string": DataType.STRING, "varchar": DataType.STRING, "text": DataType.STRING,
            "double": DataType.FLOAT64, "float64": DataType.FLOAT64, "float": DataType.FLOAT32,
            "real": DataType.FLOAT32, "bigint": DataType.INT64, "int64": DataType.INT64,
            "int": DataType.INT32, "integer": DataType.INT32, "smallint": DataType.INT16,
            "tinyint": DataType.INT8, "boolean": DataType.BOOL, "bool": DataType.BOOL,
            "uint64": DataType.UINT64, "uint32": DataType.UINT32,
            "timestamp": DataType.TIMESTAMP_MS, "timestamp(3)": DataType.TIMESTAMP_MS,
            "timestamp(9)": DataType.TIMESTAMP_NS, "datetime": DataType.TIMESTAMP_MS,
            "json": DataType.JSON,
        }
        merge_mode = str(c.options.get("merge_mode", "last_row")).lower()
        cols = []
        for i, (name, typ, opts) in enumerate(c.columns):
            tl = typ.lower()
            if tl.startswith("vector"):
                import re as _re3
                m = _re3.match(r"vector\((\d+)\)", tl)
                dim = int(m.group(1)) if m else 0
                cols.append(ColumnSchema(name, DataType.VECTOR, SemanticType.FIELD,
                                         i, vector_dim=dim))
                continue
            t = type_map.get(tl)
            if t is None:
                raise InvalidArguments(f"unknown type {typ}")
            if name == c.time_index and not t.is_timestamp:
                t = DataType.TIMESTAMP_MS
            sem = (SemanticType.TIMESTAMP if name == c.time_index
                   else SemanticType.TAG if name in c.primary_key
                   else SemanticType.FIELD)
            # string FIELD columns default to fulltext-indexed (observability
            # default; opt out via the column-less declaration in stores)
            # a last_non_null table cannot carry a fulltext index, so there
            # only an explicit FULLTEXT asks for one (and is rejected below)
            ft = opts.get("fulltext",
                          t.is_string_like and sem == SemanticType.FIELD
                          and merge_mode != "last_non_null")
            cols.append(ColumnSchema(name, t, sem, i,
                                     nullable=opts.get("nullable", True),
                                     fulltext=bool(ft)))
        schema = TableSchema(name=c.name, columns=cols, primary_key=c.primary_key,
                             options={k: v for k, v in c.options.items()})
        n_regions = c.partitions
        if c.partition_on is not None:
            from greptimedb_amd.parallel.partition import (MultiDimPartitionRule,
                                                           PartitionExpr)
            pcols, pexprs = c.partition_on
            for pc in pcols:
                if pc not in c.primary_key:
                    raise InvalidArguments(
                        f"partition column {pc} must be a primary-key (tag) column")
            rule = MultiDimPartitionRule(pcols,
                                         [PartitionExpr.from_ast(e) for e in pexprs])
            schema.options["partition_rule"] = rule.to_json()
            n_regions = rule.n_regions
        append = str(c.options.get("append_mode", "false")).lower() == "true"
        self.engine.create_table(schema, n_regions=n_regions,
                                 append_mode=append, if_not_exists=c.if_not_exists,
                                 merge_mode=merge_mode)
        return QueryResult(["status"], [["ok"]])

    def _exec_create_external(self, c: ast.CreateTable) -> QueryResult:
        """CREATE EXTERNAL TABLE … WITH (location=…, format=…) — the file
        engine (ref src/file-engine: read-only tables over files). MI355X
        take: the file is materialized into device columns at create (our
        cache policy is HBM-resident anyway); reads are then identical to
        native tables; writes are rejected."""
        import pyarrow as pa
        loc = c.options.get("location") or c.options.get("LOCATION")
        if not loc:
            raise InvalidArguments("external table needs WITH (location='…')")
        loc = str(loc).strip("'")
        fmt = str(c.options.get("format", "")).strip("'").lower() or (
            "csv" if loc.endswith(".csv") else
            "json" if loc.endswith(".json") else "parquet")
        if c.name in self.engine.tables:
            if c.if_not_exists:
                return QueryResult(["status"], [["ok"]])
            from greptimedb_amd.utils.errors import TableAlreadyExists
            raise TableAlreadyExists(c.name)
        # infer schema from the file when no column list was given
        if fmt == "parquet":
            import pyarrow.parquet as pq
            t = pq.read_table(loc)
        elif fmt == "csv":
            import pyarrow.csv as pacsv
            t = pacsv.read_csv(loc)
        else:
            import json as _json
            rows = [_json.loads(l) for l in open(loc) if l.strip()]
            t = pa.Table.from_pydict(
                {k: [r.get(k) for r in rows] for k in (rows[0] if rows else {})})
        ts_name = None
        for fld in t.schema:
            if pa.types.is_timestamp(fld.type):
                ts_name = fld.name
                break
        if ts_name is None:
            for cand in ("ts", "timestamp", "time"):
                if cand in t.column_names:
                    ts_name = cand
                    break
        if ts_name is None:
            raise InvalidArguments("external file has no timestamp column")
        cols = []
        cid = 0
        for fld in t.schema:
            if fld.name == ts_name:
                cols.append(ColumnSchema(ts_name, DataType.TIMESTAMP_MS,
                                         SemanticType.TIMESTAMP, cid))
            elif pa.types.is_string(fld.type) or pa.types.is_large_string(fld.type):
                cols.append(ColumnSchema(fld.name, DataType.STRING,
                                         SemanticType.FIELD, cid))
            else:
                cols.append(ColumnSchema(fld.name, DataType.FLOAT64,
                                         SemanticType.FIELD, cid))
            cid += 1
        schema = TableSchema(name=c.name, columns=cols, primary_key=[])
        st = self.engine.create_table(schema, n_regions=1, append_mode=True)
        st.external = True
        for region in st.regions:
            region.ensure_fields([cc.name for cc in cols
                                  if cc.semantic == SemanticType.FIELD
                                  and cc.dtype == DataType.FLOAT64])
            region.ensure_str_fields([cc.name for cc in cols
                                      if cc.dtype == DataType.STRING],
                                     fulltext=False)
        st.external = False      # let the COPY-FROM load path write
        self._exec_copy(ast.Copy(c.name, loc, "from", {"format": fmt}))
        st.external = True
        return QueryResult(["status"], [["ok"]])

    def _exec_insert(self, ins: ast.InsertValues) -> QueryResult:
        st = self.engine.table(ins.table)
        if getattr(st, "external", False):
            raise InvalidArguments(f"table {ins.table} is external (read-only)")
        schema = st.schema
        if ins.select is not None:
            # INSERT INTO t [cols] SELECT ... — positional column mapping
            # (reference: operator insert-from-query path)
            r = self.execute_stmt(ins.select)
            cols = ins.columns or r.names
            if len(cols) != len(r.names):
                raise InvalidArguments(
                    f"INSERT SELECT: {len(cols)} target columns, "
                    f"{len(r.names)} selected")
            ins = ast.InsertValues(ins.table, list(cols),
                                   [list(row) for row in r.rows()])
            return self._exec_insert(ins)
        cols = ins.columns or [c.name for c in schema.columns]
        n = len(ins.rows)
        by_col = {c: [r[i] for r in ins.rows] for i, c in enumerate(cols)}
        ts_name = schema.time_index.name
        if ts_name not in by_col:
            raise InvalidArguments("INSERT must include the time index")
        ts_ms = np.array([
            _lit_ts_ms(v, True) for v in by_col[ts_name]], dtype=np.int64)
        tag_names = [c.name for c in schema.tag_columns]
        field_names = st.regions[0].field_names
        str_names = st.regions[0].str_field_names
        new_fields = [c for c in cols
                      if c not in tag_names and c != ts_name
                      and c not in field_names and c not in str_names]
        for c in list(new_fields):
            # declared string fields, or undeclared columns with str values
            declared = schema.column(c).dtype.is_string_like if schema.has_column(c) else None
            sample = next((v for v in by_col[c] if v is not None), None)
            if declared or (declared is None and isinstance(sample, str)
                            and c not in field_names):
                str_names = str_names + [c] if c not in str_names else str_names
                new_fields.remove(c)
        if new_fields:
            for r in st.regions:
                r.ensure_fields(new_fields)
            field_names = st.regions[0].field_names
        # per-row routing
        from greptimedb_amd.engine import pk_codec
        from greptimedb_amd.engine.series import tsid_hash
        rows_by_region: dict[int, list[int]] = {}
        codes = np.empty(n, dtype=np.int32)
        regions = np.empty(n, dtype=np.int32)
        for i in range(n):
            tags = tuple(str(by_col[t][i]) if by_col.get(t) is not None and by_col[t][i] is not None
                         else None for t in tag_names)
            ridx = self.engine.region_of_tags(st, tags)
            codes[i] = st.regions[ridx].register_series(tags)
            regions[i] = ridx
            rows_by_region.setdefault(ridx, []).append(i)
        for ridx, rows in rows_by_region.items():
            rows = np.array(rows)
            fmat = np.full((len(field_names), len(rows)), np.nan)
            for j, fn in enumerate(field_names):
                if fn in by_col:
                    fmat[j] = [float(by_col[fn][r]) if by_col[fn][r] is not None else np.nan
                               for r in rows]
            def _coerce(sn, v):
                if v is None:
                    return None
                if schema.has_column(sn) and schema.column(sn).dtype == DataType.VECTOR:
                    import json as _json
                    arr = np.asarray(_json.loads(v) if isinstance(v, str) else v,
                                     dtype=np.float32)
                    return arr.tobytes()
                return v
            str_fields = {sn: [_coerce(sn, by_col[sn][r]) for r in rows]
                          for sn in str_names if sn in by_col} or None
            self.engine.write_region(st, ridx, codes[rows], ts_ms[rows], fmat, [],
                                     str_fields=str_fields)
        self.engine.commit_wal()
        return QueryResult(["status"], [[f"inserted {n}"]])

    # ---------------------------------------------------------- SELECT

    def _resolve_subqueries(self, x, outer=None):
        """Execute uncorrelated (SELECT …) nodes and splice their results in
        as literals (scalar) / literal lists (IN); equality-correlated
        scalar subqueries decorrelate into a grouped map evaluated as a
        per-series LUT (ast.CorrMap — the MergeScan-side of DataFusion's
        decorrelation)."""
        if x is None:
            return None
        if isinstance(x, ast.ScalarSubquery):
            if outer is not None and not x.many:
                corr = self._try_decorrelate(x.select, outer)
                if corr is not None:
                    return corr
            r = self._exec_select(x.select)
            col = list(r.columns[0]) if r.columns else []

            def lit(v):
                if v is None:
                    return ast.Lit(None)
                if isinstance(v, (np.floating, float)):
                    return ast.Lit(float(v))
                if isinstance(v, (np.integer, int)):
                    return ast.Lit(int(v))
                return ast.Lit(str(v))
            if x.many:
                return [lit(v) for v in col]
            return lit(col[0]) if len(col) else ast.Lit(None)
        if isinstance(x, ast.Exists):
            return self._resolve_exists(x, outer)
        if isinstance(x, ast.BinOp):
            x.left = self._resolve_subqueries(x.left, outer)
            x.right = self._resolve_subqueries(x.right, outer)
        elif isinstance(x, ast.UnaryOp):
            x.operand = self._resolve_subqueries(x.operand, outer)
        elif isinstance(x, ast.Func):
            x.args = [self._resolve_subqueries(a, outer) for a in x.args]
        elif isinstance(x, ast.Between):
            x.low = self._resolve_subqueries(x.low, outer)
            x.high = self._resolve_subqueries(x.high, outer)
        elif isinstance(x, ast.InList):
            items = []
            for it in x.items:
                got = self._resolve_subqueries(it, outer)
                items.extend(got if isinstance(got, list) else [got])
            x.items = items
        return x

    def _resolve_exists(self, x: "ast.Exists", outer):
        """EXISTS (SELECT … WHERE inner.k = outer.k AND rest) rewrites to
        `outer.k IN (SELECT inner.k WHERE rest)` (semi-join decorrelation,
        the shape DataFusion's subquery rules produce in the reference);
        uncorrelated EXISTS executes once and folds to a constant
        predicate vectorized over the outer time index."""
        inner = x.select
        corr = None
        if outer is not None and isinstance(outer.table, str) and \
                isinstance(inner.table, str) and inner.where is not None:
            outer_quals = {outer.table}
            if outer.table_alias:
                outer_quals.add(outer.table_alias)
            conjs = _split_conjuncts(inner.where)
            for i, c in enumerate(conjs):
                if not (isinstance(c, ast.BinOp) and c.op == "=" and
                        isinstance(c.left, ast.Col) and
                        isinstance(c.right, ast.Col)):
                    continue
                for a, b in ((c.left.name, c.right.name),
                             (c.right.name, c.left.name)):
                    if "." in a and a.rsplit(".", 1)[0] in outer_quals:
                        ck = b.rsplit(".", 1)[1] if "." in b else b
                        corr = (i, ck, a.rsplit(".", 1)[1])
                        break
                if corr is not None:
                    break
        if corr is not None:
            i, inner_key, outer_key = corr
            conjs = _split_conjuncts(inner.where)
            inner_quals = {inner.table}
            if inner.table_alias:
                inner_quals.add(inner.table_alias)

            def strip(e):
                """Drop inner-table qualifiers so the sub-select plans as a
                plain single-table query."""
                if isinstance(e, ast.Col) and "." in e.name and \
                        e.name.rsplit(".", 1)[0] in inner_quals:
                    return ast.Col(e.name.rsplit(".", 1)[1])
                if isinstance(e, ast.BinOp):
                    return ast.BinOp(e.op, strip(e.left), strip(e.right))
                if isinstance(e, ast.UnaryOp):
                    return ast.UnaryOp(e.op, strip(e.operand))
                if isinstance(e, ast.Func):
                    return ast.Func(e.name, [strip(a) for a in e.args],
                                    e.distinct)
                if isinstance(e, ast.InList):
                    return ast.InList(strip(e.expr),
                                      [strip(a) for a in e.items], e.negated)
                if isinstance(e, ast.Between):
                    return ast.Between(strip(e.expr), strip(e.low),
                                       strip(e.high), e.negated)
                if isinstance(e, ast.IsNull):
                    return ast.IsNull(strip(e.expr), e.negated)
                return e
            rest = [strip(c) for j, c in enumerate(conjs) if j != i]
            w2 = None
            for c in rest:
                w2 = c if w2 is None else ast.BinOp("and", w2, c)
            sub = ast.Select(projections=[(ast.Col(inner_key), None)],
                             table=inner.table,
                             table_alias=inner.table_alias, where=w2)
            items = self._resolve_subqueries(
                ast.ScalarSubquery(sub, many=True), None)
            return ast.InList(ast.Col(outer_key), items,
                              negated=x.negated)
        r = self._exec_select(inner)
        nonempty = bool(r.columns and len(r.columns[0]))
        truth = nonempty != x.negated
        if outer is not None and isinstance(outer.table, str) and \
                outer.table in self.engine.tables:
            ts_name = self.engine.table(outer.table).schema.time_index.name
            # ts is never NULL: IS NOT NULL ≡ always-true, IS NULL ≡ false
            return ast.IsNull(ast.Col(ts_name), negated=truth)
        return ast.Lit(truth)

    def _try_decorrelate(self, inner: ast.Select, outer: ast.Select):
        """`(SELECT agg(x) FROM t2 [t2a] WHERE t2.k = o.k AND ...)` with the
        outer qualifier matching `outer`'s table/alias → grouped map.
        Returns ast.CorrMap or None (not correlated / unsupported)."""
        if not isinstance(inner.table, str) or inner.where is None or \
                not isinstance(outer.table, str):
            return None
        if len(inner.projections) != 1:
            return None
        proj, _a = inner.projections[0]
        if not (isinstance(proj, ast.Func) and proj.name in AGG_FUNCS):
            return None
        outer_quals = {outer.table}
        if outer.table_alias:
            outer_quals.add(outer.table_alias)
        inner_quals = {inner.table}
        if inner.table_alias:
            inner_quals.add(inner.table_alias)

        def split(e, out):
            if isinstance(e, ast.BinOp) and e.op == "and":
                split(e.left, out)
                split(e.right, out)
            else:
                out.append(e)
        conjs: list = []
        split(inner.where, conjs)
        corr_idx = inner_key = outer_key = None
        for i, c in enumerate(conjs):
            if not (isinstance(c, ast.BinOp) and c.op == "=" and
                    isinstance(c.left, ast.Col) and isinstance(c.right, ast.Col)):
                continue
            for a, b in ((c.left.name, c.right.name),
                         (c.right.name, c.left.name)):
                if "." in a:
                    qa, ca = a.rsplit(".", 1)
                    if qa in outer_quals:
                        cb = b.rsplit(".", 1)[1] if "." in b else b
                        corr_idx, inner_key, outer_key = i, cb, ca
                        break
            if corr_idx is not None:
                break
        if corr_idx is None:
            return None
        rest = [c for i, c in enumerate(conjs) if i != corr_idx]
        where2 = None
        for c in rest:
            where2 = c if where2 is None else ast.BinOp("and", where2, c)
        grouped = ast.Select(
            projections=[(ast.Col(inner_key), "__k"), (proj, "__v")],
            table=inner.table, table_alias=inner.table_alias,
            where=where2, group_by=[ast.Col(inner_key)])
        r = self._exec_select(grouped)
        keys = list(r.columns[0]) if r.columns else []
        vals = list(r.columns[1]) if len(r.columns) > 1 else []
        m = {None if k is None else str(k):
             (float(v) if v is not None else float("nan"))
             for k, v in zip(keys, vals)}
        return ast.CorrMap(m, outer_key)

    def _exec_select(self, sel: ast.Select) -> QueryResult:
        if sel.ctes:
            return self._with_ctes(sel)
        if isinstance(sel.table, ast.ValuesTable):
            # FROM (VALUES ...) t(a, b) — literal rows as a derived table
            from greptimedb_amd.query.derived import select_over_result
            vt = sel.table
            width = max((len(r) for r in vt.rows), default=0)
            names2 = list(vt.columns) if vt.columns else                 [f"column{i+1}" for i in range(width)]
            cols2 = [[r[i] if i < len(r) else None for r in vt.rows]
                     for i in range(width)]
            base = QueryResult(names2, cols2)
            return select_over_result(sel, base)
        if isinstance(sel.table, (ast.Select, ast.SetOp)):
            # derived table: FROM (SELECT ...) alias
            from greptimedb_amd.query.derived import select_over_result
            base = self.execute_stmt(sel.table)
            return select_over_result(sel, base)
        if isinstance(sel.table, str):
            vt = self._virtual.get(sel.table)
            if vt is None:
                view_sql = getattr(self.engine, "views", {}).get(sel.table)
                if view_sql is not None:
                    vt = self.execute(view_sql)
            if vt is not None:
                from greptimedb_amd.query.derived import select_over_result
                return select_over_result(sel, vt)
        if _has_subquery(sel.where) or _has_subquery(sel.having) or \
                any(_has_subquery(e) for e, _a in sel.projections):
            sel.projections = [(self._resolve_subqueries(e, sel), a)
                               for e, a in sel.projections]
            sel.where = self._resolve_subqueries(sel.where, sel)
            sel.having = self._resolve_subqueries(sel.having, sel)
        has_moments = isinstance(sel.table, str) and \
            sel.table in self.engine.tables and \
            self._has_sketch_agg(sel, self._MOMENT_AGGS)
        if has_moments and sel.joins:
            return self._exec_join_aggregate(sel)
        if isinstance(sel.table, str) and sel.table in self.engine.tables \
                and (has_moments or self._has_sketch_agg(sel)):
            dq = self._plan_device_quantile(sel)
            if dq is not None:
                try:
                    return self._exec_device_quantile(dq)
                except PlanQuery:
                    pass    # a shape the planner let through: host path
            return self._exec_sketch_select(sel)
        if sel.table is None:
            # constant select
            names, cols = [], []
            for i, (e, alias) in enumerate(sel.projections):
                v = self._eval_session_const(e)
                names.append(alias or _expr_name(e) if not isinstance(
                    e, (ast.Lit,)) else (alias or f"col{i}"))
                cols.append([v])
            return QueryResult(names, cols)
        from greptimedb_amd.query.information_schema import is_information_schema
        if is_information_schema(sel.table):
            return self._exec_information_schema(sel)
        if sel.joins:
            return self._exec_join(sel)
        try:
            plan = self._plan_select(sel)
            if any(_has_range_agg(e) for e, _a in sel.projections):
                return self._exec_range_select(sel, plan)
            if plan.aggs:
                return self._exec_aggregate(sel, plan)
            knn = self._try_vector_knn(sel, plan)
            if knn is not None:
                return knn
            return self._exec_raw(sel, plan)
        except PlanQuery:
            return self._select_fallback(sel)

    def _select_fallback(self, sel: ast.Select) -> QueryResult:
        """General-shape fallback: shapes the fused device planner rejects
        (aggregates over expressions like sum(CASE WHEN …), ORDER BY
        expressions, …) materialize the WHERE-filtered raw rows once and
        evaluate through the derived-table engine (reference parity:
        DataFusion handles these generically; our device planner covers
        the hot TSBS/observability shapes and this path covers the tail)."""
        if not (isinstance(sel.table, str) and sel.table in self.engine.tables):
            raise PlanQuery(f"unsupported select shape on {sel.table!r}")
        if getattr(sel, "_in_fallback", False):
            raise PlanQuery("unsupported select shape (fallback failed)")
        from greptimedb_amd.query.derived import select_over_result
        inner = ast.Select(projections=[(ast.Star(), None)], table=sel.table,
                           where=sel.where)
        inner._in_fallback = True
        base = self._exec_select(inner)
        outer = ast.Select(projections=sel.projections, table=None,
                           where=None, group_by=sel.group_by,
                           having=sel.having, order_by=sel.order_by,
                           limit=sel.limit, offset=sel.offset)
        return select_over_result(outer, base)

    def _exec_join(self, sel: ast.Select) -> QueryResult:
        """Two-table equality JOIN (inner/left): each side runs as a pushed-
        down raw scan, then a host-side hash join (reference: DataFusion
        HashJoinExec; time-series queries rarely join, so host-side is the
        right cost tier)."""
        if len(sel.joins) != 1:
            raise PlanQuery("only single JOIN supported")
        j = sel.joins[0]
        sides = {
            (sel.table_alias or sel.table): sel.table,
            (j.alias or j.table): j.table,
        }
        aliases = list(sides)
        if len(sides) != 2:
            raise PlanQuery("join sides must have distinct aliases")

        def side_columns(alias):
            st = self.engine.table(sides[alias])
            cols = {c.name for c in st.schema.columns}
            cols.update(st.regions[0].field_names)
            cols.update(st.regions[0].str_field_names)
            return cols

        side_cols = {a: side_columns(a) for a in aliases}

        def resolve(name):
            """'a.x' or unqualified 'x' → (alias, col)."""
            if "." in name:
                a, c = name.split(".", 1)
                if a in sides:
                    return a, c
            owners = [a for a in aliases if name in side_cols[a]]
            if len(owners) == 1:
                return owners[0], name
            raise PlanQuery(f"ambiguous or unknown join column {name!r}")

        # ON: equality conjuncts across sides
        pairs = []
        for c in _split_conjuncts(j.on):
            if not (isinstance(c, ast.BinOp) and c.op == "=" and
                    isinstance(c.left, ast.Col) and isinstance(c.right, ast.Col)):
                raise PlanQuery("JOIN ON supports column equality conjuncts")
            la, lc = resolve(c.left.name)
            ra, rc = resolve(c.right.name)
            if la == ra:
                raise PlanQuery("JOIN ON must compare columns across sides")
            if la == aliases[0]:
                pairs.append((lc, rc))
            else:
                pairs.append((rc, lc))

        # WHERE: push side-local conjuncts down; cross-side unsupported
        side_where = {a: [] for a in aliases}
        if sel.where is not None:
            for c in _split_conjuncts(sel.where):
                refs = {resolve(n)[0] for n in _expr_cols(c)}
                if len(refs) != 1:
                    raise PlanQuery("cross-side WHERE predicates unsupported")
                a = next(iter(refs))

                def strip(e):
                    if isinstance(e, ast.Col):
                        return ast.Col(resolve(e.name)[1])
                    if isinstance(e, ast.BinOp):
                        return ast.BinOp(e.op, strip(e.left), strip(e.right))
                    if isinstance(e, ast.UnaryOp):
                        return ast.UnaryOp(e.op, strip(e.operand))
                    if isinstance(e, ast.InList):
                        return ast.InList(strip(e.expr), e.items, e.negated)
                    if isinstance(e, ast.Between):
                        return ast.Between(strip(e.expr), e.low, e.high, e.negated)
                    if isinstance(e, ast.Func):
                        return ast.Func(e.name, [strip(x) for x in e.args])
                    return e
                side_where[a].append(strip(c))

        # needed columns per side
        need = {a: set() for a in aliases}
        out_spec = []  # (alias_out_name, side, col)
        for e, al in sel.projections:
            if isinstance(e, ast.Star):
                for a in aliases:
                    for c in sorted(side_cols[a]):
                        out_spec.append((f"{a}.{c}", a, c))
                        need[a].add(c)
                continue
            if not isinstance(e, ast.Col):
                raise PlanQuery("JOIN projections: columns or *")
            a, c = resolve(e.name)
            out_spec.append((al or e.name, a, c))
            need[a].add(c)
        for lc, rc in pairs:
            need[aliases[0]].add(lc)
            need[aliases[1]].add(rc)
        order_resolved = []
        for e, desc in sel.order_by:
            if not isinstance(e, ast.Col):
                raise PlanQuery("JOIN ORDER BY: columns only")
            a, c = resolve(e.name)
            need[a].add(c)
            order_resolved.append((a, c, desc))

        # execute sides as raw scans — build (right) side first
        data = {}
        la, ra = aliases

        def run_side(a):
            w = None
            for c in side_where[a]:
                w = c if w is None else ast.BinOp("and", w, c)
            sub = ast.Select([(ast.Col(c), None) for c in sorted(need[a])],
                             sides[a], where=w)
            r = self.execute_stmt(sub)
            data[a] = {n: np.asarray(col)
                       for n, col in zip(r.names, r.columns)}

        run_side(ra)
        # C10 dynamic filter (reference dist_plan remote_dyn_filter_*): on
        # INNER joins push the build side's distinct key values into the
        # probe side's scan predicate — in distributed mode the gathered
        # build keys act as the broadcast filter, shrinking every rank's
        # probe materialization before the gather.
        if j.kind == "inner" and len(pairs) == 1:
            rvals = data[ra][pairs[0][1]]
            uniq = {v for v in rvals.tolist() if v is not None}
            if len(uniq) <= 65536:
                side_where[la].append(ast.InList(
                    ast.Col(pairs[0][0]),
                    [ast.Lit(v) for v in sorted(uniq, key=str)]))
        run_side(la)

        def keys_of(a, cols):
            arrs = [data[a][c] for c in cols]
            n = len(arrs[0]) if arrs else 0
            return [tuple(x[i] for x in arrs) for i in range(n)]

        lkeys = keys_of(la, [p[0] for p in pairs])
        rkeys = keys_of(ra, [p[1] for p in pairs])
        rindex: dict = {}
        for i, k in enumerate(rkeys):
            rindex.setdefault(k, []).append(i)
        li, ri = [], []
        for i, k in enumerate(lkeys):
            hits = rindex.get(k)
            if hits:
                for h in hits:
                    li.append(i)
                    ri.append(h)
            elif j.kind == "left":
                li.append(i)
                ri.append(-1)
        li = np.asarray(li, dtype=np.int64)
        ri = np.asarray(ri, dtype=np.int64)

        names, cols, kinds = [], [], []
        for name, a, c in out_spec:
            src = data[a][c]
            if a == la:
                vals = src[li] if len(li) else src[:0]
            else:
                vals = np.array([src[x] if x >= 0 else None for x in ri],
                                dtype=object)
            names.append(name)
            cols.append(vals)
            ts_col = self.engine.table(sides[a]).schema.time_index.name
            kinds.append("ts" if c == ts_col else "")
        n_out = len(li)
        idx = np.arange(n_out)
        for a, c, desc in reversed(order_resolved):
            arr = (data[a][c][li] if a == la else
                   np.array([data[a][c][x] if x >= 0 else None for x in ri],
                            dtype=object))
            o = np.argsort(arr[idx], kind="stable")
            idx = idx[o[::-1] if desc else o]
        if sel.offset:
            idx = idx[sel.offset:]
        if sel.limit is not None:
            idx = idx[: sel.limit]
        return QueryResult(names, [c[idx] for c in cols], kinds)

    VEC_FUNCS = {"vec_cos_distance": "cos", "vec_l2sq_distance": "l2sq",
                 "vec_dot_product": "dot"}

    def _try_vector_knn(self, sel: ast.Select, plan: SelectPlan):
        """kNN fast path (reference: src/index vector/HNSW + vec_* UDFs).

        SELECT ..., vec_*_distance(col, '[..]') AS d ... ORDER BY d LIMIT k
        → brute-force distances over device-resident vectors (matmul /
        cdist on HBM — at MI355X bandwidth this beats CPU HNSW well past
        10M vectors) + per-source topk + global merge."""
        import json as _json
        dist_expr = alias = None
        for e, a in sel.projections:
            if isinstance(e, ast.Func) and e.name in self.VEC_FUNCS:
                dist_expr, alias = e, a
        if dist_expr is None or sel.limit is None or len(sel.order_by) != 1:
            return None
        oe, desc = sel.order_by[0]
        targets = {alias} if alias else set()
        if not ((isinstance(oe, ast.Col) and oe.name in targets) or
                _same_expr(oe, dist_expr)):
            return None
        mode = self.VEC_FUNCS[dist_expr.name]
        if (mode == "dot") != desc:
            return None  # dot ranks descending; distances ascending
        if not (isinstance(dist_expr.args[0], ast.Col) and
                isinstance(dist_expr.args[1], ast.Lit)):
            return None
        vcol = dist_expr.args[0].name
        q = torch.as_tensor(np.asarray(_json.loads(dist_expr.args[1].value),
                                       dtype=np.float32))
        st = plan.table
        device = self.engine.config.device
        q = q.to(device)
        k = sel.limit
        ts_lo = plan.ts_lo if plan.ts_lo is not None else -(1 << 62)
        ts_hi = plan.ts_hi if plan.ts_hi is not None else (1 << 62)
        out_cols = [(e, a) for e, a in sel.projections if e is not dist_expr]

        cands = []  # (dist, source, row)
        for region in st.regions:
            cand = self._candidate_codes(region, plan)
            lut = None
            if cand is not None:
                lut = np.full(len(region.series), -1, dtype=np.int32)
                lut[np.asarray(cand, dtype=np.int64)] = 1
            lut_t = torch.as_tensor(lut, device=device) if lut is not None else None
            for src in region.scan_sources(ts_lo, ts_hi):
                col = src.str_cols.get(vcol)
                if col is None:
                    continue
                # build/cache the [n, D] device tensor from packed bytes
                # (cached on the SstBatch; memtable sources rebuild per query)
                cache_holder = None
                key = f"_vec_{vcol}"
                vt = None
                for b in region.sst_cache.values():
                    if b.ts is src.ts:
                        vt = getattr(b, key, None)
                        cache_holder = b
                        break
                if vt is None:
                    blob = b"".join(v if v is not None else b"" for v in col)
                    flat = np.frombuffer(blob, dtype=np.float32)
                    lens = np.array([0 if v is None else len(v) // 4 for v in col])
                    if len(set(lens[lens > 0])) > 1:
                        raise PlanQuery("inconsistent vector dimensions")
                    D = int(lens.max()) if len(lens) else 0
                    if D == 0:
                        continue
                    full = np.full((len(col), D), np.nan, dtype=np.float32)
                    full[lens > 0] = flat.reshape(-1, D)
                    vt = torch.as_tensor(full).to(device)
                    if cache_holder is not None:
                        setattr(cache_holder, key, vt)
                mask = filter_series_time(src.ts, src.series, lut_t, ts_lo, ts_hi)
                if plan.residual is not None:
                    mask &= self._eval_mask(plan.residual, src, region, device)
                qf = q.float()
                # IVF-flat probe when ADMIN build_vector_index attached one
                # to this (SST) source; memtable sources stay brute-force
                ivf = getattr(cache_holder, f"_ivf_{vcol}", None) \
                    if cache_holder is not None else None
                rows_sub = None
                vt_d = vt
                if ivf is not None:
                    from greptimedb_amd.vector import ivf_candidates
                    nprobe = getattr(region, "vector_index", {}).get(
                        vcol, {}).get("nprobe", 16)
                    rows_sub = ivf_candidates(ivf, qf, nprobe)
                    vt_d = vt[rows_sub]
                if mode == "l2sq":
                    d = ((vt_d - qf[None, :]) ** 2).sum(dim=1)
                elif mode == "cos":
                    d = 1.0 - (vt_d @ qf) / (vt_d.norm(dim=1) * qf.norm() + 1e-30)
                else:
                    d = -(vt_d @ qf)  # dot: negate so smaller = better
                m = mask if rows_sub is None else mask[rows_sub]
                bad = ~m | torch.isnan(d)
                d = torch.where(bad, torch.full_like(d, float("inf")), d)
                kk = min(k, d.numel())
                if kk == 0:
                    continue
                vals, idx = torch.topk(d, kk, largest=False)
                if rows_sub is not None:
                    idx = rows_sub[idx]
                vh = vals.cpu().numpy()
                ih = idx.cpu().numpy()
                for dist, row in zip(vh, ih):
                    if np.isfinite(dist):
                        cands.append((float(dist), region, src, int(row)))
        cands.sort(key=lambda x: x[0])
        cands = cands[:k]

        names, cols, kinds = [], [], []
        ts_name = st.schema.time_index.name
        for e, a in sel.projections:
            if e is dist_expr:
                dvals = [(-c[0] if mode == "dot" else c[0]) for c in cands]
                names.append(a or _expr_name(e))
                cols.append(np.asarray(dvals))
                kinds.append("")
                continue
            if not isinstance(e, ast.Col):
                raise PlanQuery("vector knn projections: columns + distance")
            vals = []
            for _d, region, src, row in cands:
                if e.name == ts_name:
                    vals.append(int(src.ts[row]))
                elif e.name in region.series.tag_names:
                    code = int(src.series[row])
                    vals.append(region.series.tag_array(e.name)[code])
                elif e.name in src.field_pos:
                    vals.append(float(src.fields[src.field_pos[e.name]][row]))
                elif e.name in src.str_cols:
                    v = src.str_cols[e.name][row]
                    if isinstance(v, (bytes, bytearray)) and e.name != vcol:
                        v = v.decode(errors="replace")
                    elif isinstance(v, (bytes, bytearray)):
                        v = np.frombuffer(v, dtype=np.float32).round(4).tolist()
                    vals.append(v)
                else:
                    vals.append(None)
            names.append(a or e.name)
            cols.append(np.asarray(vals, dtype=object))
            kinds.append("ts" if e.name == ts_name else "")
        return QueryResult(names, cols, kinds)

    def _exec_information_schema(self, sel: ast.Select) -> QueryResult:
        from greptimedb_amd.query import information_schema as isch
        names, cols = isch.build(self.engine, sel.table)
        n = len(cols[0]) if cols else 0
        data = dict(zip(names, cols))
        keep = np.ones(n, dtype=bool)
        if sel.where is not None:
            def ev(e):
                if isinstance(e, ast.BinOp) and e.op == "and":
                    return ev(e.left) & ev(e.right)
                if isinstance(e, ast.BinOp) and e.op == "or":
                    return ev(e.left) | ev(e.right)
                if isinstance(e, ast.BinOp) and e.op in ("=", "!=", "<", "<=", ">", ">="):
                    l, r = e.left, e.right
                    if isinstance(l, ast.Col) and isinstance(r, ast.Lit):
                        col = data[l.name]
                        return np.array([_py_cmp(e.op, v, r.value) for v in col])
                raise PlanQuery("information_schema WHERE supports simple comparisons")
            keep = ev(sel.where)
        idx = np.flatnonzero(keep)
        out_names, out_cols = [], []
        for e, alias in sel.projections:
            if isinstance(e, ast.Star):
                out_names.extend(names)
                out_cols.extend([data[c][idx] for c in names])
            elif isinstance(e, ast.Col):
                out_names.append(alias or e.name)
                out_cols.append(data[e.name][idx])
            else:
                raise PlanQuery("information_schema projections: columns / *")
        if sel.order_by:
            o = np.arange(len(idx))
            for e, desc in reversed(sel.order_by):
                a = data[e.name][idx][o]
                oo = np.argsort(a, kind="stable")
                o = o[oo[::-1] if desc else oo]
            out_cols = [c[o] for c in out_cols]
        if sel.limit is not None:
            out_cols = [c[: sel.limit] for c in out_cols]
        return QueryResult(out_names, out_cols)

    def _qualify_names(self, stmt):
        """Schema-qualify table names via the session (reference:
        QueryContext current_schema resolution)."""
        if self.session.schema == "public":
            return
        res = self.session.resolve_table
        def fix_select(sel):
            if isinstance(sel, ast.SetOp):
                fix_select(sel.left)
                fix_select(sel.right)
                return
            if not isinstance(sel, ast.Select):
                return
            cte_names = {n for n, _q in sel.ctes}
            for _n, q in sel.ctes:
                fix_select(q)
            if isinstance(sel.table, str):
                from greptimedb_amd.query.information_schema import \
                    is_information_schema
                if sel.table not in cte_names and \
                        sel.table not in self._virtual and \
                        not is_information_schema(sel.table):
                    sel.table = res(sel.table)
            elif sel.table is not None:
                fix_select(sel.table)
            for j in sel.joins:
                j.table = res(j.table)
        if isinstance(stmt, (ast.Select, ast.SetOp)):
            fix_select(stmt)
        elif isinstance(stmt, ast.CreateTable):
            stmt.name = res(stmt.name)
        elif isinstance(stmt, (ast.DropTable, ast.ShowCreateTable,
                               ast.DescribeTable, ast.TruncateTable)):
            stmt.name = res(stmt.name)
        elif isinstance(stmt, ast.InsertValues):
            stmt.table = res(stmt.table)
            if stmt.select is not None:
                fix_select(stmt.select)
        elif isinstance(stmt, ast.Delete):
            stmt.table = res(stmt.table)
        elif isinstance(stmt, ast.AlterTable):
            stmt.table = res(stmt.table)

    _SKETCH_AGGS = {"hll", "hll_merge", "uddsketch_state", "uddsketch_merge",
                    "approx_percentile", "median", "hll_count",
                    "uddsketch_calc"}

    # two-pass second-moment aggregates -> argument count
    _MOMENT_AGGS = MOMENT_KINDS

    def _has_sketch_agg(self, sel, names=None) -> bool:
        """Whether projections or HAVING call one of `names` (default: the
        sketch aggregates); such statements leave the fused planner."""
        names = self._SKETCH_AGGS if names is None else names

        def walk(e):
            if isinstance(e, ast.Func):
                if e.name.lower() in names:
                    return True
                return any(walk(a) for a in e.args)
            if isinstance(e, ast.BinOp):
                return walk(e.left) or walk(e.right)
            if isinstance(e, ast.UnaryOp):
                return walk(e.operand)
            return False
        return any(walk(e) for e, _a in sel.projections) or \
            (sel.having is not None and walk(sel.having))

    def _exec_join_aggregate(self, sel: ast.Select) -> QueryResult:
        """Moment aggregates over a JOIN: the join runs as a plain select of
        every referenced column and the derived evaluator aggregates its
        rows, as _exec_sketch_select does for a single table."""
        import dataclasses

        from greptimedb_amd.query.derived import select_over_result
        aliases = {a for _e, a in sel.projections if a}
        exprs = [e for e, _a in sel.projections] + list(sel.group_by) + \
            [e for e, _d in sel.order_by]
        if sel.having is not None:
            exprs.append(sel.having)
        needed = sorted(set().union(*[_expr_cols(e) for e in exprs]) - aliases)
        if not needed:
            raise PlanQuery("aggregate over a JOIN references no column")
        inner = ast.Select(projections=[(ast.Col(c), None) for c in needed],
                           table=sel.table, table_alias=sel.table_alias,
                           joins=sel.joins, where=sel.where)
        base = self._exec_join(inner)
        outer = dataclasses.replace(sel, table=None, table_alias=None,
                                    joins=[], where=None)
        return select_over_result(outer, base)

    def _exec_sketch_select(self, sel: ast.Select) -> QueryResult:
        """Sketch/approx aggregates (hll / uddsketch / approx_percentile):
        materialize the referenced raw columns (GPU scan + filter), then
        aggregate via the derived evaluator (reference: DataFusion runs
        these UDAFs over the scanned batches the same way)."""
        import dataclasses

        from greptimedb_amd.query.derived import select_over_result
        st = self.engine.table(sel.table)
        region0 = st.regions[0]
        table_cols = ({c.name for c in st.schema.columns} |
                      set(region0.field_names) |
                      set(region0.str_field_names) |
                      {st.schema.time_index.name})
        needed: set = set()

        # time-bucket calls (GROUP BY date_bin(...)) are not something the
        # derived evaluator knows: lift each into a hidden "ts"-kind column
        # computed from the time index, named after the call it replaces
        ts_name = st.schema.time_index.name
        buckets: dict = {}      # repr(call) -> (hidden column, BucketSpec)

        def lift(e):
            if isinstance(e, ast.Func) and e.name in BUCKET_FUNCS:
                if repr(e) not in buckets:
                    buckets[repr(e)] = (f"__bucket{len(buckets)}",
                                        self._bucket_spec(e, ts_name))
                return ast.Col(buckets[repr(e)][0])
            if isinstance(e, ast.Func):
                return ast.Func(e.name, [lift(a) for a in e.args], e.distinct)
            if isinstance(e, ast.BinOp):
                return ast.BinOp(e.op, lift(e.left), lift(e.right))
            if isinstance(e, ast.UnaryOp):
                return ast.UnaryOp(e.op, lift(e.operand))
            return e

        def has_bucket(e):
            if isinstance(e, ast.Func):
                return e.name in BUCKET_FUNCS or any(has_bucket(a) for a in e.args)
            if isinstance(e, ast.BinOp):
                return has_bucket(e.left) or has_bucket(e.right)
            if isinstance(e, ast.UnaryOp):
                return has_bucket(e.operand)
            return False

        if any(has_bucket(e) for e in
               [e for e, _a in sel.projections] + list(sel.group_by) +
               [e for e, _d in sel.order_by] +
               ([sel.having] if sel.having is not None else [])):
            from greptimedb_amd.query.derived import _name_of
            sel = dataclasses.replace(
                sel,
                projections=[(lift(e), a or (_name_of(e, i) if has_bucket(e)
                                             else None))
                             for i, (e, a) in enumerate(sel.projections)],
                group_by=[lift(g) for g in sel.group_by],
                having=lift(sel.having) if sel.having is not None else None,
                order_by=[(lift(e), d) for e, d in sel.order_by])
            needed.add(ts_name)

        def collect(e):
            if isinstance(e, ast.Col) and e.name in table_cols:
                needed.add(e.name)
            elif isinstance(e, ast.Func):
                for a in e.args:
                    collect(a)
            elif isinstance(e, ast.BinOp):
                collect(e.left)
                collect(e.right)
            elif isinstance(e, ast.UnaryOp):
                collect(e.operand)
        for e, _a in sel.projections:
            collect(e)
        for g in sel.group_by:
            collect(g)
        if sel.having is not None:
            collect(sel.having)
        for e, _d in sel.order_by:
            collect(e)
        if not needed:
            needed.add(st.schema.time_index.name)
        base_sel = ast.Select(
            projections=[(ast.Col(c), None) for c in sorted(needed)],
            table=sel.table, table_alias=sel.table_alias, where=sel.where)
        base = self._exec_select(base_sel)
        if buckets:
            ts_col = np.asarray(base.columns[base.names.index(ts_name)],
                                dtype=np.int64)
            names, columns, kinds = (list(base.names), list(base.columns),
                                     list(base.kinds))
            for hidden, spec in buckets.values():
                o = spec.origin or 0
                names.append(hidden)
                columns.append(o + (ts_col - o) // spec.bucket_ms * spec.bucket_ms)
                kinds.append("ts")
            base = QueryResult(names, columns, kinds)
        outer = dataclasses.replace(sel, table=None, table_alias=None,
                                    where=None)
        return select_over_result(outer, base)

    # ------------------------------------------- device percentiles (K21)

    # Class switches, like Ingestor._fused: False keeps approx_percentile /
    # median, respectively the var / stddev / covar / corr family, on the
    # materialising host path (_exec_sketch_select).
    _device_quantile = True
    _device_moments = True

    def _plan_device_quantile(self, sel: ast.Select):
        """Device plan for approx_percentile(field, p) / median(field) and
        the moment aggregates (var_pop(field) ... corr(field, field)),
        grouped by tags and/or one time bucket, or None when the statement
        has to stay on the host path. Nothing is scanned here."""
        import dataclasses
        from greptimedb_amd.ops.cpu_ref import MAX_QUANTILE_CELLS
        if self.dist is not None:
            return None
        if not (isinstance(sel.table, str) and sel.table in self.engine.tables
                and (self._has_sketch_agg(sel) or
                     self._has_sketch_agg(sel, self._MOMENT_AGGS))):
            return None
        if sel.joins or sel.distinct or sel.ctes or sel.align_ms is not None:
            return None
        st = self.engine.table(sel.table)
        float_fields = {c.name for c in st.schema.field_columns
                        if c.dtype.is_float} & \
            set(st.regions[0].field_names)

        sels: dict[str, tuple[str, float]] = {}   # repr(call) -> (field, p)
        moms: dict[str, tuple[str, str, str]] = {}  # repr(call) -> (fn, x, y)
        agg_args: set = set()      # fields under sum/avg/min/max

        def walk(e, in_agg):
            """False as soon as the expression leaves the supported shape."""
            if isinstance(e, (ast.Lit, ast.Col, ast.Star, ast.Interval)):
                return True
            if isinstance(e, ast.BinOp):
                return walk(e.left, in_agg) and walk(e.right, in_agg)
            if isinstance(e, ast.UnaryOp):
                return walk(e.operand, in_agg)
            if not isinstance(e, ast.Func):
                return False
            fn = e.name.lower()
            if fn in self._MOMENT_AGGS:
                if in_agg or e.distinct or len(e.args) != self._MOMENT_AGGS[fn]:
                    return False
                if not all(isinstance(a, ast.Col) and a.name in float_fields
                           for a in e.args):
                    return False
                moms[repr(e)] = (fn, e.args[0].name, e.args[-1].name)
                return True
            if fn in self._SKETCH_AGGS:
                if in_agg or e.distinct or fn not in ("approx_percentile", "median"):
                    return False
                if len(e.args) != (2 if fn == "approx_percentile" else 1):
                    return False
                col = e.args[0]
                if not (isinstance(col, ast.Col) and col.name in float_fields):
                    return False
                p = 0.5
                if fn == "approx_percentile":
                    try:
                        p = _eval_const(e.args[1])
                    except Exception:
                        return False
                    if isinstance(p, bool) or not isinstance(p, (int, float)):
                        return False
                    p = float(p)
                    if not 0.0 <= p <= 1.0:
                        return False
                sels[repr(e)] = (col.name, p)
                return True
            if e.name in AGG_FUNCS and e.name != "count" and e.args and \
                    isinstance(e.args[0], ast.Col):
                agg_args.add(e.args[0].name)
            nested = in_agg or e.name in AGG_FUNCS
            return all(walk(a, nested) for a in e.args)

        def positional(e):
            if isinstance(e, ast.Lit) and isinstance(e.value, int) and \
                    not isinstance(e.value, bool) and \
                    1 <= e.value <= len(sel.projections):
                return sel.projections[e.value - 1][0]
            return e

        group_by = [positional(g) for g in sel.group_by]
        order_by = [(positional(e), d) for e, d in sel.order_by]
        if any(isinstance(e, ast.Star) for e, _a in sel.projections):
            return None
        exprs = [e for e, _a in sel.projections] + [e for e, _d in order_by]
        if sel.having is not None:
            exprs.append(sel.having)
        if not all(walk(e, False) for e in exprs) or not (sels or moms):
            return None
        if (sels and not self._device_quantile) or \
                (moms and not self._device_moments):
            return None
        if any(_has_range_agg(e) for e in exprs) or \
                any(_collect_window_nodes(e, w := []) or w for e in exprs):
            return None
        # GROUP BY keys and ORDER BY expressions ride along as hidden
        # projections: _plan_select then collects their aggregates, and the
        # result is ordered afterwards the way the host path orders it. One
        # hidden count(field) per aggregated field tells NULL (no value in
        # the group) from a NaN that the arithmetic produced.
        # A moment call's NULL mask is pairwise, so it travels as a plane of
        # its own: one hidden marker call per moment call, which
        # _exec_device_quantile resolves through extra_planes.
        null_fields = sorted({f for f, _p in sels.values()} | agg_args)
        m_calls = list(moms)
        hidden = [(g, None) for g in group_by] + \
            [(e, None) for e, _d in order_by] + \
            [(ast.Func("count", [ast.Col(f)]), None) for f in null_fields] + \
            [(_moment_null_marker(i), None) for i in range(len(m_calls))]
        sel2 = dataclasses.replace(
            sel, projections=list(sel.projections) + hidden, group_by=group_by,
            order_by=[], limit=None, offset=None)
        try:
            plan = self._plan_select(sel2)
            if any(a.func in ("last_value", "first_value", "count_distinct")
                   for a in plan.aggs):
                return None
            grid = self._agg_time_grid(plan)
        except PlanQuery:
            return None
        # ordinary aggregates read the f64 field matrix: anything else
        # (count(ts), max(tag), an unknown column) stays on the host path
        numeric = set(st.regions[0].field_names)
        if any(a.arg is not None and a.arg not in numeric for a in plan.aggs):
            return None
        aliases = {a for _e, a in sel.projections if a}

        def finalizable(e):
            """What _finalize_agg can evaluate over group rows."""
            if isinstance(e, ast.Lit):
                return True
            if isinstance(e, ast.Col):
                return e.name in aliases or e.name in plan.group_tags
            if isinstance(e, ast.BinOp):
                return finalizable(e.left) and finalizable(e.right)
            if isinstance(e, ast.UnaryOp):
                return finalizable(e.operand)
            if isinstance(e, ast.Func):
                return repr(e) in sels or repr(e) in moms or \
                    e.name in AGG_FUNCS or (
                    plan.bucket_expr is not None and
                    _same_expr(e, plan.bucket_expr))
            return False
        if not all(finalizable(e) for e in exprs):
            return None
        group_keys, region_luts = self._build_group_luts(st, plan, plan.group_tags)
        n_slots = max(len(group_keys), 1)
        calls = list(sels)
        m_pairs = sorted({(x, y) for _fn, x, y in moms.values()})
        if max(len(calls), len(m_pairs)) * n_slots * grid[4] > MAX_QUANTILE_CELLS:
            return None
        return _DeviceQuantilePlan(
            sel=sel, sel2=sel2, plan=plan, grid=grid, group_keys=group_keys,
            region_luts=region_luts, n_slots=n_slots, calls=calls,
            field_of_call=[sels[c][0] for c in calls],
            p_of_sel=[sels[c][1] for c in calls],
            n_group=len(group_by), order_desc=[d for _e, d in order_by],
            null_fields=null_fields, m_calls=m_calls,
            m_kinds=[moms[c][0] for c in m_calls],
            m_sel_of_call=[m_pairs.index(moms[c][1:]) for c in m_calls],
            m_pairs=m_pairs)

    def _exec_device_quantile(self, dq) -> QueryResult:
        """Percentiles and moments where the data lives: per source one
        bucket-cell pass feeds the fused aggregate (ordinary aggregates, row
        counts), the radix-histogram selection and the two-pass moments; only
        [Q, cells] and [M, cells] planes reach the host.
        Output mirrors _exec_sketch_select: names, kinds, float-or-None
        values, rows ordered by group key unless ORDER BY says otherwise."""
        from greptimedb_amd.ops import (bucket_cells, grouped_moments,
                                        grouped_quantile, moments_finish,
                                        quantile_lerp, ts_bucket_agg_acc,
                                        ts_bucket_agg_finish)
        from greptimedb_amd.query.derived import _contains_agg, _name_of
        plan, sel = dq.plan, dq.sel
        st = plan.table
        device = self.engine.config.device
        ts_lo, ts_hi, origin, bucket_ms, n_buckets = dq.grid
        n_slots = dq.n_slots
        agg_fields = sorted({a.arg for a in plan.aggs if a.arg is not None} |
                            set(dq.field_of_call) |
                            {f for pair in dq.m_pairs for f in pair})
        nf = len(agg_fields)
        field_of_sel = [agg_fields.index(f) for f in dq.field_of_call]
        n_q, n_m = len(dq.calls), len(dq.m_calls)

        # The cell ids (4 B per row) and, for merge-mode or residual-filtered
        # regions, the deduplicated field copies of every source stay alive
        # across the nine passes, next to the histogram.
        acc = None
        sources = []
        for region, lut in zip(st.regions, dq.region_luts):
            self._cancel_check()
            lut_t = torch.as_tensor(lut, device=device)
            for ts_t, se_t, f_t, fidx_t in self._region_agg_inputs(
                    region, plan, device, agg_fields, ts_lo, ts_hi):
                acc = ts_bucket_agg_acc(ts_t, se_t, f_t, fidx_t, lut_t,
                                        ts_lo, ts_hi, origin, bucket_ms,
                                        n_slots, n_buckets, acc=acc)
                cell = bucket_cells(ts_t, se_t, lut_t, ts_lo, ts_hi, origin,
                                    bucket_ms, n_buckets)
                sources.append((cell, f_t, fidx_t))
        self._cancel_check()
        shape = (n_slots, n_buckets)
        if acc is None:
            sums = np.zeros((nf,) + shape)
            cnts = np.zeros((nf,) + shape, dtype=np.int64)
            mins = np.full((nf,) + shape, np.nan)
            maxs = np.full((nf,) + shape, np.nan)
            rowcnt = np.zeros(shape, dtype=np.int64)
            qvals = np.full((n_q,) + shape, np.nan)
            mvals = np.full((n_m,) + shape, np.nan)
            mnull = np.ones((n_m,) + shape)
        else:
            qvals = np.full((n_q,) + shape, np.nan)
            if n_q:
                lo, hi, cnt = grouped_quantile(
                    sources, field_of_sel, dq.p_of_sel, n_slots * n_buckets,
                    on_pass=self._cancel_check)
                qvals = quantile_lerp(lo.cpu().numpy(), hi.cpu().numpy(),
                                      cnt.cpu().numpy(), dq.p_of_sel)
                qvals = qvals.reshape((n_q,) + shape)
            mvals = np.full((n_m,) + shape, np.nan)
            mnull = np.ones((n_m,) + shape)
            if n_m:
                planes = [t.cpu().numpy() for t in grouped_moments(
                    sources, [agg_fields.index(x) for x, _y in dq.m_pairs],
                    [agg_fields.index(y) for _x, y in dq.m_pairs],
                    n_slots * n_buckets)]
                for i, (kind, s) in enumerate(zip(dq.m_kinds, dq.m_sel_of_call)):
                    val, null = moments_finish(kind, [p[s] for p in planes])
                    mvals[i] = val.reshape(shape)
                    mnull[i] = null.reshape(shape)
            sums, cnts, mins, maxs, rowcnt = [
                t.cpu().numpy() for t in ts_bucket_agg_finish(acc)]
        del sources
        plane_of = {c: qvals[i] for i, c in enumerate(dq.calls)}
        plane_of.update({c: mvals[i] for i, c in enumerate(dq.m_calls)})
        plane_of.update({repr(_moment_null_marker(i)): mnull[i]
                         for i in range(n_m)})
        field_of = dict(zip(dq.calls, dq.field_of_call))

        res = self._finalize_agg(
            dq.sel2, plan, dq.group_keys, origin, bucket_ms, agg_fields,
            sums, cnts, mins, maxs, rowcnt,
            extra_planes=lambda e: plane_of.get(repr(e)))

        # order, cut and format the way the host path does
        n_vis = len(sel.projections)
        n_ord = len(dq.order_desc)
        cols = [np.asarray(c) for c in res.columns]
        m = len(cols[0]) if cols else 0
        gcols = cols[n_vis:n_vis + dq.n_group]
        o0 = n_vis + dq.n_group
        cnt_of = dict(zip(dq.null_fields, cols[o0 + n_ord:]))
        mnull_of = dict(zip(dq.m_calls,
                            cols[o0 + n_ord + len(dq.null_fields):]))
        alias_expr = {a: e for e, a in sel.projections if a}

        def null_mask(e):
            """Rows where the host path yields None: an aggregate over a
            group without a non-NULL value, or arithmetic on one."""
            if isinstance(e, ast.Lit):
                return np.full(m, e.value is None)
            if isinstance(e, ast.Col) and e.name in alias_expr:
                return null_mask(alias_expr[e.name])
            if isinstance(e, ast.BinOp):
                return null_mask(e.left) | null_mask(e.right)
            if isinstance(e, ast.UnaryOp):
                return null_mask(e.operand)
            if isinstance(e, ast.Func) and repr(e) in field_of:
                return cnt_of[field_of[repr(e)]] == 0
            if isinstance(e, ast.Func) and repr(e) in mnull_of:
                return mnull_of[repr(e)].astype(np.float64) != 0
            if isinstance(e, ast.Func) and e.name in AGG_FUNCS and \
                    e.name != "count" and isinstance(e.args[0], ast.Col):
                return cnt_of[e.args[0].name] == 0
            return np.zeros(m, dtype=bool)

        def rank(col, e, desc=False):
            """Sort codes of one key column: value order, NULL/NaN last
            (first when descending), as derived._sort_key orders them."""
            if col.dtype == object:
                null = np.array([v is None for v in col], dtype=bool)
            else:
                null = np.isnan(col) if col.dtype.kind == "f" else \
                    np.zeros(m, dtype=bool)
            null = null | null_mask(e)
            code = np.zeros(m, dtype=np.int64)
            if not null.all():
                _u, inv = np.unique(col[~null], return_inverse=True)
                code[~null] = inv
                code[null] = int(inv.max()) + 1
            return -code if desc else code

        hidden = dq.sel2.projections
        idx = np.arange(m)
        if gcols and m:
            idx = np.lexsort(tuple(
                rank(g, hidden[n_vis + i][0])
                for i, g in reversed(list(enumerate(gcols)))))
        if n_ord and m:
            keys = [rank(cols[o0 + i], hidden[o0 + i][0], dq.order_desc[i])[idx]
                    for i in range(n_ord)]
            idx = idx[np.lexsort(tuple(reversed(keys)))]
        if sel.offset:
            idx = idx[sel.offset:]
        if sel.limit is not None:
            idx = idx[: sel.limit]
        names, out, kinds = [], [], []
        for pi, (e, a) in enumerate(sel.projections):
            names.append(a or _name_of(e, pi))
            kinds.append(res.kinds[pi])
            if _contains_agg(e):
                vals = cols[pi].astype(np.float64)[idx]
                null = null_mask(e)[idx]
                if null.any():
                    vals = vals.astype(object)
                    vals[null] = None
                out.append(list(vals))
            else:
                out.append(list(cols[pi][idx]))
        return QueryResult(names, out, kinds)

    def _with_ctes(self, stmt):

        """Evaluate WITH ctes into the virtual-table scope, then run the
        body (reference: DataFusion CTE planning; cases in tests/cases/cte)."""
        import dataclasses
        saved = dict(self._virtual)
        try:
            for name, q in stmt.ctes:
                self._virtual[name] = self.execute_stmt(q)
            body = dataclasses.replace(stmt, ctes=[])
            return self.execute_stmt(body)
        finally:
            self._virtual = saved

    def _exec_setop(self, so: "ast.SetOp") -> QueryResult:
        from greptimedb_amd.query.derived import eval_setop, select_over_result
        if so.ctes:
            return self._with_ctes(so)
        left = self.execute_stmt(so.left)
        right = self.execute_stmt(so.right)
        res = eval_setop(so.op, so.all, left, right)
        if so.order_by or so.limit is not None:
            wrap = ast.Select(projections=[(ast.Star(), None)], table=None,
                              order_by=so.order_by, limit=so.limit)
            res = select_over_result(wrap, res)
        return res

    def _exec_create_view(self, cv: "ast.CreateView") -> QueryResult:
        """CREATE [OR REPLACE] VIEW name AS select (reference:
        common/meta ddl create_view; view body stored verbatim and
        re-planned per query like the reference's logical-plan views)."""
        views = getattr(self.engine, "views", None)
        if views is None:
            views = self.engine.views = {}
        if cv.name in views and not cv.or_replace:
            if cv.if_not_exists:
                return QueryResult(["status"], [["ok"]])
            raise TableAlreadyExists(cv.name)
        if cv.name in self.engine.tables:
            raise TableAlreadyExists(cv.name)
        self.execute(cv.query_sql)   # validate the body now
        views[cv.name] = cv.query_sql
        self.engine._save_catalog()
        return QueryResult(["status"], [["ok"]])

    def _plan_select(self, sel: ast.Select) -> SelectPlan:
        st = self.engine.table(sel.table)
        schema = st.schema
        ts_name = schema.time_index.name
        tag_names = {c.name for c in schema.tag_columns}
        alias_map = {alias: e for e, alias in sel.projections if alias}

        # WHERE analysis
        ts_lo = ts_hi = None
        tag_conj = []
        residual = []
        if sel.where is not None:
            sel.where = _fold_const_casts(sel.where)
            for c in _split_conjuncts(sel.where):
                done = False
                if isinstance(c, ast.BinOp) and c.op in ("<", "<=", ">", ">=", "="):
                    l, r, op = c.left, c.right, c.op
                    if isinstance(r, ast.Col) and isinstance(l, ast.Lit):
                        l, r = r, l
                        op = {"<": ">", "<=": ">=", ">": "<", ">=": "<="}.get(op, op)
                    if isinstance(l, ast.Col) and isinstance(r, ast.Lit):
                        if l.name == ts_name:
                            v = _lit_ts_ms(r.value, True)
                            if op == ">=":
                                ts_lo = v if ts_lo is None else max(ts_lo, v)
                            elif op == ">":
                                ts_lo = v + 1 if ts_lo is None else max(ts_lo, v + 1)
                            elif op == "<":
                                ts_hi = v if ts_hi is None else min(ts_hi, v)
                            elif op == "<=":
                                ts_hi = v + 1 if ts_hi is None else min(ts_hi, v + 1)
                            elif op == "=":
                                ts_lo, ts_hi = v, v + 1
                            done = True
                        elif l.name in tag_names and op == "=":
                            tag_conj.append((l.name, [str(r.value)]))
                            done = True
                elif isinstance(c, ast.InList) and not c.negated and \
                        isinstance(c.expr, ast.Col) and c.expr.name in tag_names and \
                        all(isinstance(i, ast.Lit) for i in c.items):
                    tag_conj.append((c.expr.name, [str(i.value) for i in c.items]))
                    done = True
                elif isinstance(c, ast.Between) and not c.negated and \
                        isinstance(c.expr, ast.Col) and c.expr.name == ts_name and \
                        isinstance(c.low, ast.Lit) and isinstance(c.high, ast.Lit):
                    lo = _lit_ts_ms(c.low.value, True)
                    hi = _lit_ts_ms(c.high.value, True) + 1
                    ts_lo = lo if ts_lo is None else max(ts_lo, lo)
                    ts_hi = hi if ts_hi is None else min(ts_hi, hi)
                    done = True
                if not done:
                    residual.append(c)
        residual_expr = None
        if residual:
            residual_expr = residual[0]
            for c in residual[1:]:
                residual_expr = ast.BinOp("and", residual_expr, c)

        # GROUP BY analysis
        bucket = bucket_expr = None
        group_tags = []
        for g in sel.group_by:
            if isinstance(g, ast.Col) and g.name in alias_map:
                g = alias_map[g.name]
            if isinstance(g, ast.Col):
                if g.name in tag_names:
                    group_tags.append(g.name)
                else:
                    raise PlanQuery(f"GROUP BY on non-tag column {g.name} unsupported")
            elif isinstance(g, ast.Func) and g.name in BUCKET_FUNCS:
                bucket, bucket_expr = self._bucket_spec(g, ts_name), g
            else:
                raise PlanQuery(f"unsupported GROUP BY expr {g}")

        # aggregates in projections / having / order
        aggs = []

        def collect(e):
            if isinstance(e, ast.Func) and e.name in AGG_FUNCS:
                if e.distinct and e.name == "count" and len(e.args) == 1 and \
                        isinstance(e.args[0], ast.Col) and e.args[0].name in tag_names:
                    aggs.append(AggCall("count_distinct", e.args[0].name))
                elif len(e.args) == 1 and isinstance(e.args[0], ast.Star):
                    aggs.append(AggCall("count", None))
                elif len(e.args) == 1 and isinstance(e.args[0], ast.Col):
                    fname = "avg" if e.name == "mean" else e.name
                    aggs.append(AggCall(fname, e.args[0].name))
                else:
                    raise PlanQuery(f"unsupported aggregate {e}")
            elif isinstance(e, ast.BinOp):
                collect(e.left); collect(e.right)
            elif isinstance(e, ast.UnaryOp):
                collect(e.operand)
            elif isinstance(e, ast.Func):
                for a in e.args:
                    collect(a)
        for e, _ in sel.projections:
            collect(e)
        if sel.having is not None:
            collect(sel.having)

        return SelectPlan(
            table=st, ts_lo=ts_lo, ts_hi=ts_hi, tag_conj=tag_conj,
            residual=residual_expr, bucket=bucket, bucket_expr=bucket_expr,
            group_tags=group_tags, aggs=aggs, projections=sel.projections,
            order_by=sel.order_by, having=sel.having, limit=sel.limit,
            offset=sel.offset)

    def _bucket_spec(self, f: ast.Func, ts_name: str) -> BucketSpec:
        if f.name == "date_trunc":
            if len(f.args) != 2 or not isinstance(f.args[0], ast.Lit):
                raise PlanQuery("date_trunc(unit, ts) expected")
            unit = trunc_unit_ms(str(f.args[0].value))
            if unit is None:
                raise PlanQuery(f"unsupported date_trunc unit {f.args[0].value}")
            origin = None
            tz = getattr(self.session, "tz_offset_ms", 0)
            if tz and unit >= 3_600_000:
                # session time zone shifts the truncation grid (local
                # midnight != UTC midnight; reference QueryContext timezone)
                origin = (-tz) % unit
            return BucketSpec(bucket_ms=unit, origin=origin)
        # date_bin(interval, ts[, origin]) / time_bucket(interval, ts)
        if not f.args or not isinstance(f.args[0], (ast.Interval, ast.Lit)):
            raise PlanQuery("date_bin(interval, ts) expected")
        arg0 = f.args[0]
        if isinstance(arg0, ast.Interval):
            ms = arg0.ms
        else:
            from greptimedb_amd.query.parser import parse_interval_text
            ms = parse_interval_text(str(arg0.value))
        origin = None
        if f.name == "date_bin" and len(f.args) > 2 and isinstance(f.args[2], ast.Lit):
            origin = _lit_ts_ms(f.args[2].value, True)
        return BucketSpec(bucket_ms=ms, origin=origin)

    # ------------------------------------------------------ aggregate path

    def _candidate_codes(self, region, plan: SelectPlan):
        """Codes passing the conjunctive tag predicates (None = all)."""
        codes = None
        for tag, values in plan.tag_conj:
            got = set(region.series.codes_for_in(tag, values))
            codes = got if codes is None else (codes & got)
        if codes is None:
            return None
        return sorted(codes)

    def _build_group_luts(self, st, plan, gt):
        """Per-region code→group-slot LUTs + global group-key dict.

        Vectorized over the tag-value dictionary (factor codes), not per
        series — high-cardinality GROUP BY tags stay off the Python path."""
        group_keys: dict[tuple, int] = {}
        region_luts = []
        for region in st.regions:
            cand = self._candidate_codes(region, plan)
            nser = len(region.series)
            lut = np.full(nser, -1, dtype=np.int32)
            sel_idx = np.arange(nser) if cand is None else \
                np.asarray(cand, dtype=np.int64)
            if gt:
                if len(sel_idx):
                    key = np.zeros(len(sel_idx), dtype=np.int64)
                    mult = 1
                    factors = []
                    for t in gt:
                        codes_arr, values = region.series.tag_codes(t)
                        factors.append((codes_arr, values))
                        card = len(values) + 1
                        if mult > (1 << 62) // max(card, 1):
                            _, key = np.unique(key, return_inverse=True)
                            mult = int(key.max()) + 1 if len(key) else 1
                        key = key + (codes_arr[sel_idx].astype(np.int64) + 1) * mult
                        mult *= card
                    uniq, first, inv = np.unique(key, return_index=True,
                                                 return_inverse=True)
                    slots_of_uniq = np.empty(len(uniq), dtype=np.int32)
                    for u in range(len(uniq)):
                        code = int(sel_idx[first[u]])
                        kt = tuple(values[codes_arr[code]] if codes_arr[code] >= 0
                                   else None
                                   for codes_arr, values in factors)
                        slots_of_uniq[u] = group_keys.setdefault(kt, len(group_keys))
                    lut[sel_idx] = slots_of_uniq[inv]
            else:
                lut[sel_idx] = 0
                group_keys.setdefault((), 0)
            region_luts.append(lut)
        return group_keys, region_luts

    def _agg_time_grid(self, plan: SelectPlan):
        """(ts_lo, ts_hi, origin, bucket_ms, n_buckets) of an aggregate
        plan: open time bounds close on the regions' data range, the bucket
        grid starts at the bucket holding ts_lo."""
        st = plan.table
        ts_lo, ts_hi = plan.ts_lo, plan.ts_hi
        if ts_lo is None or ts_hi is None:
            lo = hi = None
            for r in st.regions:
                tr = r.time_range()
                if tr:
                    lo = tr[0] if lo is None else min(lo, tr[0])
                    hi = tr[1] if hi is None else max(hi, tr[1])
            if self.dist is not None:
                lo, hi = self.dist.minmax_ts(lo, hi)
            if lo is None:
                lo, hi = 0, 1
            else:
                hi = hi + 1
            ts_lo = ts_lo if ts_lo is not None else lo
            ts_hi = ts_hi if ts_hi is not None else hi
        if plan.bucket is not None:
            bucket_ms = plan.bucket.bucket_ms
            origin = plan.bucket.origin
            if origin is None:
                origin = (ts_lo // bucket_ms) * bucket_ms
            else:
                origin += ((ts_lo - origin) // bucket_ms) * bucket_ms
            n_buckets = int((ts_hi - 1 - origin) // bucket_ms) + 1
            if n_buckets > MAX_BUCKETS:
                raise PlanQuery(f"too many time buckets: {n_buckets}")
        else:
            bucket_ms = max(int(ts_hi - ts_lo), 1)
            origin = ts_lo
            n_buckets = 1
        return ts_lo, ts_hi, origin, bucket_ms, n_buckets

    def _exec_aggregate(self, sel: ast.Select, plan: SelectPlan) -> QueryResult:
        if any(a.func in ("last_value", "first_value") for a in plan.aggs):
            return self._exec_lastpoint(sel, plan)
        st = plan.table
        device = self.engine.config.device

        ts_lo, ts_hi, origin, bucket_ms, n_buckets = self._agg_time_grid(plan)

        # count(DISTINCT tag): group by (outer tags + distinct tag) internally,
        # then collapse effective groups back to outer groups at finalize
        dtags = sorted({a.arg for a in plan.aggs if a.func == "count_distinct"})
        if len(dtags) > 1:
            raise PlanQuery("only one count(DISTINCT tag) per query")
        eff_gt = list(plan.group_tags) + [t for t in dtags
                                          if t not in plan.group_tags]
        group_keys, region_luts = self._build_group_luts(st, plan, eff_gt)
        n_slots = max(len(group_keys), 1)

        # fields needed
        agg_fields = sorted({a.arg for a in plan.aggs if a.arg is not None})
        nf = len(agg_fields)

        from greptimedb_amd.ops import ts_bucket_agg_acc, ts_bucket_agg_finish
        acc = None  # opaque accumulator handle (GPU: shared atomic buffers)
        for region, lut in zip(st.regions, region_luts):
            self._cancel_check()
            lut_t = torch.as_tensor(lut, device=device)
            for ts_t, se_t, f_t, fidx_t in self._region_agg_inputs(
                    region, plan, device, agg_fields, ts_lo, ts_hi):
                acc = ts_bucket_agg_acc(ts_t, se_t, f_t, fidx_t, lut_t,
                                        ts_lo, ts_hi, origin, bucket_ms,
                                        n_slots, n_buckets, acc=acc)
        if acc is None:
            z = torch.zeros
            final = [z((nf, n_slots, n_buckets), dtype=torch.float64),
                     z((nf, n_slots, n_buckets), dtype=torch.int64),
                     torch.full((nf, n_slots, n_buckets), float("nan"), dtype=torch.float64),
                     torch.full((nf, n_slots, n_buckets), float("nan"), dtype=torch.float64),
                     z((n_slots, n_buckets), dtype=torch.int64)]
        else:
            final = ts_bucket_agg_finish(acc)

        sums, cnts, mins, maxs, rowcnt = [t.cpu().numpy() for t in final]

        if self.dist is not None:
            group_keys, (sums, cnts, mins, maxs, rowcnt) = self.dist.merge_groups(
                group_keys, sums, cnts, mins, maxs, rowcnt)
            n_slots = max(len(group_keys), 1)

        distinct_plane = None
        if dtags:
            # collapse effective groups (outer × distinct tag) → outer groups
            n_out_tags = len(plan.group_tags)
            outer_keys: dict[tuple, int] = {}
            eff_to_outer = np.zeros(max(len(group_keys), 1), dtype=np.int64)
            for key, slot in group_keys.items():
                ok = tuple(key[:n_out_tags])
                eff_to_outer[slot] = outer_keys.setdefault(ok, len(outer_keys))
            n_outer = max(len(outer_keys), 1)
            nb = rowcnt.shape[1]
            new_sums = np.zeros((sums.shape[0], n_outer, nb))
            new_cnts = np.zeros((cnts.shape[0], n_outer, nb), dtype=np.int64)
            new_mins = np.full((mins.shape[0], n_outer, nb), np.nan)
            new_maxs = np.full((maxs.shape[0], n_outer, nb), np.nan)
            new_rows = np.zeros((n_outer, nb), dtype=np.int64)
            distinct_plane = np.zeros((n_outer, nb), dtype=np.int64)
            for s in range(rowcnt.shape[0]):
                o = eff_to_outer[s]
                new_sums[:, o] += np.where(cnts[:, s] > 0, sums[:, s], 0.0)
                new_cnts[:, o] += cnts[:, s]
                new_mins[:, o] = np.fmin(new_mins[:, o], mins[:, s])
                new_maxs[:, o] = np.fmax(new_maxs[:, o], maxs[:, s])
                new_rows[o] += rowcnt[s]
                distinct_plane[o] += (rowcnt[s] > 0).astype(np.int64)
            sums, cnts, mins, maxs, rowcnt = (new_sums, new_cnts, new_mins,
                                              new_maxs, new_rows)
            group_keys = outer_keys

        return self._finalize_agg(sel, plan, group_keys, origin, bucket_ms,
                                  agg_fields, sums, cnts, mins, maxs, rowcnt,
                                  distinct_plane=distinct_plane, dtag=(dtags[0] if dtags else None))

    def _exec_lastpoint(self, sel: ast.Select, plan: SelectPlan) -> QueryResult:
        """TSBS `lastpoint` shape: last_value(field) per group (latest-ts row).

        Reference parity: DISTINCT ON / last_value window in the reference's
        TSBS adapter. Per region: per-slot argmax over ts, then value-at-max;
        regions/ranks combine by ts comparison (groups are series-aligned so
        at most one shard owns a group in the common case)."""
        st = plan.table
        device = self.engine.config.device
        if plan.bucket is not None:
            raise PlanQuery("last_value with time buckets unsupported")
        funcs = {a.func for a in plan.aggs}
        if len(funcs) != 1:
            raise PlanQuery("cannot mix last_value with other aggregates")
        # first_value = argmin over ts: run the same argmax machinery on
        # negated timestamps (merge/dist combine logic is sign-agnostic)
        rev = funcs == {"first_value"}
        lv_fields = sorted({a.arg for a in plan.aggs})
        ts_lo = plan.ts_lo if plan.ts_lo is not None else -(1 << 62)
        ts_hi = plan.ts_hi if plan.ts_hi is not None else (1 << 62)
        sl_lo, sl_hi = (-ts_hi, -ts_lo) if rev else (ts_lo, ts_hi)

        gt = plan.group_tags
        group_keys, region_luts = self._build_group_luts(st, plan, gt)
        best_ts: np.ndarray | None = None
        best_val: np.ndarray | None = None

        for region, lut in zip(st.regions, region_luts):
            self._cancel_check()
            lut_t = torch.as_tensor(lut, device=device)
            sources = region.scan_sources(ts_lo, ts_hi)
            if plan.residual is not None:
                # rare: pre-filter sources through the residual mask
                filt = []
                for src in sources:
                    mask = self._eval_mask(plan.residual, src, region, device)
                    idx = mask.nonzero(as_tuple=True)[0]
                    if idx.numel():
                        filt.append((src, idx))
                pairs = [((-src.ts[idx]).contiguous() if rev
                          else src.ts[idx].contiguous(),
                          src.series[idx].contiguous(),
                          False if rev else src.sorted)
                         for src, idx in filt]
                src_objs = [(src, idx) for src, idx in filt]
            else:
                pairs = [((-src.ts).contiguous() if rev else src.ts,
                          src.series, False if rev else src.sorted)
                         for src in sources]
                src_objs = [(src, None) for src in sources]
            if not pairs:
                continue
            ng = len(group_keys) if group_keys else 1
            from greptimedb_amd.ops import series_last
            b_ts, b_src, b_row = series_last(pairs, lut_t, sl_lo, sl_hi, ng)
            mx_h = b_ts.numpy().astype(np.int64)
            # gather winner values per source
            vals = torch.full((len(lv_fields), ng), float("nan"),
                              dtype=torch.float64, device=device)
            for si, (src, idx) in enumerate(src_objs):
                slots_here = (b_src == si).nonzero(as_tuple=True)[0]
                if slots_here.numel() == 0:
                    continue
                rows = b_row[slots_here]
                if idx is not None:
                    rows = idx.cpu()[rows]
                rows_d = rows.to(device)
                slots_d = slots_here.to(device)
                for fi, fn in enumerate(lv_fields):
                    p = src.field_pos.get(fn)
                    if p is not None:
                        vals[fi, slots_d] = src.fields[p][rows_d]
            vals_h = vals.cpu().numpy()
            mx_h = np.where(b_src.numpy() >= 0, mx_h, -(1 << 62))
            if best_ts is None:
                best_ts, best_val = mx_h, vals_h
            else:
                if len(mx_h) > len(best_ts):
                    pad = len(mx_h) - len(best_ts)
                    best_ts = np.concatenate([best_ts, np.full(pad, -(1 << 62), dtype=np.int64)])
                    best_val = np.concatenate(
                        [best_val, np.full((len(lv_fields), pad), np.nan)], axis=1)
                newer = mx_h > best_ts[: len(mx_h)]
                best_ts[: len(mx_h)][newer] = mx_h[newer]
                best_val[:, : len(mx_h)][:, newer] = vals_h[:, newer]
        ng = max(len(group_keys), 1)
        if best_ts is None:
            best_ts = np.full(ng, -(1 << 62), dtype=np.int64)
            best_val = np.full((len(lv_fields), ng), np.nan)
        elif len(best_ts) < ng:
            pad = ng - len(best_ts)
            best_ts = np.concatenate([best_ts, np.full(pad, -(1 << 62), dtype=np.int64)])
            best_val = np.concatenate([best_val, np.full((len(lv_fields), pad), np.nan)], axis=1)

        if self.dist is not None:
            group_keys, best_ts, best_val = self.dist.merge_lastpoint(
                group_keys, best_ts, best_val)
            ng = max(len(group_keys), 1)

        keys_by_slot = [None] * ng
        for k, s in group_keys.items():
            keys_by_slot[s] = k
        valid = best_ts > -(1 << 62)
        slot_idx = np.flatnonzero(valid)
        fpos = {fn: i for i, fn in enumerate(lv_fields)}

        names, cols, kinds = [], [], []
        for e, alias in plan.projections:
            if isinstance(e, ast.Col) and e.name in gt:
                i = gt.index(e.name)
                arr = np.array([keys_by_slot[s][i] for s in slot_idx], dtype=object)
                names.append(alias or e.name); cols.append(arr); kinds.append("")
            elif isinstance(e, ast.Func) and e.name in ("last_value",
                                                        "first_value"):
                arr = best_val[fpos[e.args[0].name]][slot_idx]
                names.append(alias or _expr_name(e)); cols.append(arr); kinds.append("")
            else:
                raise PlanQuery(f"unsupported lastpoint projection {e}")
        n_out = len(slot_idx)
        # ORDER BY group tags only
        idx = np.arange(n_out)
        for e, desc in reversed(plan.order_by):
            if isinstance(e, ast.Col):
                if e.name in gt:
                    i = gt.index(e.name)
                    a = np.array([keys_by_slot[s][i] for s in slot_idx], dtype=object)[idx]
                elif e.name in dict(zip(names, cols)):
                    a = np.asarray(dict(zip(names, cols))[e.name])[idx]
                else:
                    raise PlanQuery("lastpoint ORDER BY must use group tags")
                o = np.argsort(a, kind="stable")
                idx = idx[o[::-1] if desc else o]
        if plan.limit is not None:
            idx = idx[: plan.limit]
        return QueryResult(names, [np.asarray(c, dtype=object)[idx] for c in cols], kinds)

    def _region_agg_inputs(self, region, plan, device, agg_fields, ts_lo, ts_hi):
        """Yield (ts, series, fields[nf,n], field_idx) kernel inputs for one
        region. Append-mode tables: sources stream straight to the kernel.
        Merge-mode tables: sources are gathered, (series, ts, arrival)-sorted
        and LastRow-deduped first (reference read/dedup.rs semantics) so
        duplicate points don't double-count."""
        nf = len(agg_fields)
        st_append = getattr(region, "append_mode", False)
        sources = region.scan_sources(ts_lo, ts_hi)

        def source_cols(src):
            """(ts, series, fields aligned to agg_fields) after residual mask."""
            ts_t, se_t, sel_idx = src.ts, src.series, None
            if plan.residual is not None:
                mask = self._eval_mask(plan.residual, src, region, device)
                sel_idx = mask.nonzero(as_tuple=True)[0]
                ts_t = ts_t[sel_idx].contiguous()
                se_t = se_t[sel_idx].contiguous()
            m = ts_t.numel()
            f_t = torch.stack(src.take_fields(sel_idx, agg_fields)) if nf else \
                torch.zeros((1, max(m, 1)), dtype=torch.float64, device=device)
            return ts_t, se_t, f_t.contiguous()

        fidx_t = torch.arange(nf, dtype=torch.int32, device=device) if nf else \
            torch.zeros(0, dtype=torch.int32, device=device)

        if st_append or len(sources) <= 1:
            single = len(sources) == 1 and not st_append
            for src in sources:
                if plan.residual is None and src.field_pos and all(
                        fn in src.field_pos for fn in agg_fields) and not single:
                    # zero-copy: use the source's own field matrix + index map
                    fidx = torch.as_tensor(
                        np.array([src.field_pos[fn] for fn in agg_fields], dtype=np.int32),
                        device=device)
                    yield src.ts, src.series, src.fields, (
                        fidx if nf else torch.zeros(0, dtype=torch.int32, device=device))
                    continue
                ts_t, se_t, f_t = source_cols(src)
                if ts_t.numel() == 0:
                    continue
                if single:
                    # one source, merge-mode: dedup within it
                    ts_t, se_t, f_t, _, _ = sort_last_rows(se_t, ts_t, f_t)
                yield ts_t, se_t, f_t.contiguous(), fidx_t
            return
        # merge-mode, multiple sources: gather + global dedup
        cols = [source_cols(s) for s in sources]
        cols = [c for c in cols if c[0].numel()]
        if not cols:
            return
        ts_t = torch.cat([c[0] for c in cols])
        se_t = torch.cat([c[1] for c in cols])
        f_t = torch.cat([c[2] for c in cols], dim=1)
        ts_t, se_t, f_t, _, _ = sort_last_rows(se_t, ts_t, f_t)
        yield ts_t, se_t, f_t.contiguous(), fidx_t

    def _finalize_agg(self, sel, plan, group_keys, origin, bucket_ms,
                      agg_fields, sums, cnts, mins, maxs, rowcnt,
                      distinct_plane=None, dtag=None,
                      extra_planes=None) -> QueryResult:
        """`extra_planes(func_expr)`, when given, may resolve a function
        call the fused aggregates do not know (a percentile) to its
        [n_slots, n_buckets] plane; it returns None for any other call."""
        # cells with data
        slot_idx, bucket_idx = np.nonzero(rowcnt)
        if len(slot_idx) == 0 and not plan.group_tags and plan.bucket is None:
            # aggregate without GROUP BY always yields one row (count=0)
            slot_idx = np.array([0])
            bucket_idx = np.array([0])
        order = np.argsort(bucket_idx * max(len(group_keys), 1) + slot_idx, kind="stable") \
            if len(slot_idx) else np.array([], dtype=np.int64)
        slot_idx, bucket_idx = slot_idx[order], bucket_idx[order]
        n_out = len(slot_idx)
        bucket_ts = origin + bucket_idx * bucket_ms
        keys_by_slot = [None] * max(len(group_keys), 1)
        for k, s in group_keys.items():
            keys_by_slot[s] = k
        fpos = {fn: i for i, fn in enumerate(agg_fields)}

        def agg_array(func, arg):
            if func == "count_distinct":
                return distinct_plane[slot_idx, bucket_idx]
            if func == "count" and arg is None:
                return rowcnt[slot_idx, bucket_idx]
            fi = fpos[arg]
            if func == "count":
                return cnts[fi, slot_idx, bucket_idx]
            if func == "sum":
                s = sums[fi, slot_idx, bucket_idx].copy()
                s[cnts[fi, slot_idx, bucket_idx] == 0] = np.nan
                return s
            if func in ("avg", "mean"):
                c = cnts[fi, slot_idx, bucket_idx]
                with np.errstate(invalid="ignore", divide="ignore"):
                    return np.where(c > 0, sums[fi, slot_idx, bucket_idx] / c, np.nan)
            if func == "min":
                return mins[fi, slot_idx, bucket_idx]
            if func == "max":
                return maxs[fi, slot_idx, bucket_idx]
            raise PlanQuery(f"agg {func}")

        gt = plan.group_tags

        def eval_expr(e):
            """Evaluate a projection/having/order expr over group rows →
            (array, kind)."""
            if isinstance(e, ast.Lit):
                return np.full(n_out, e.value, dtype=object if isinstance(e.value, str) else None), ""
            if isinstance(e, ast.Col):
                # alias reference?
                for pe, alias in plan.projections:
                    if alias == e.name:
                        return eval_expr(pe)
                if plan.bucket_expr is not None and _same_expr(e, plan.bucket_expr):
                    return bucket_ts, "ts"
                if e.name in gt:
                    i = gt.index(e.name)
                    return np.array([keys_by_slot[s][i] for s in slot_idx], dtype=object), ""
                raise PlanQuery(f"column {e.name} not in GROUP BY")
            if isinstance(e, ast.Func):
                if plan.bucket_expr is not None and _same_expr(e, plan.bucket_expr):
                    return bucket_ts, "ts"
                if extra_planes is not None:
                    plane = extra_planes(e)
                    if plane is not None:
                        return plane[slot_idx, bucket_idx], ""
                if e.name in AGG_FUNCS:
                    if len(e.args) == 1 and isinstance(e.args[0], ast.Star):
                        return agg_array("count", None), ""
                    if e.distinct and e.name == "count" and \
                            isinstance(e.args[0], ast.Col) and e.args[0].name == dtag:
                        return agg_array("count_distinct", dtag), ""
                    fname = "avg" if e.name == "mean" else e.name
                    return agg_array(fname, e.args[0].name), ""
                raise PlanQuery(f"unsupported function {e.name} in aggregate query")
            if isinstance(e, ast.BinOp):
                l, _ = eval_expr(e.left)
                r, _ = eval_expr(e.right)
                return _np_binop(e.op, l, r), ""
            if isinstance(e, ast.UnaryOp):
                v, k = eval_expr(e.operand)
                if e.op == "-":
                    return -v, k
                return ~v.astype(bool), ""
            raise PlanQuery(f"unsupported expr {e}")

        keep = np.ones(n_out, dtype=bool)
        if plan.having is not None:
            hv, _ = eval_expr(plan.having)
            keep &= np.asarray(hv, dtype=bool)

        names, cols, kinds = [], [], []
        for i, (e, alias) in enumerate(plan.projections):
            arr, kind = eval_expr(e)
            names.append(alias or _expr_name(e))
            cols.append(np.asarray(arr))
            kinds.append(kind)

        # ORDER BY
        if plan.order_by:
            sort_cols = []
            for e, desc in reversed(plan.order_by):
                arr, _ = eval_expr(e)
                arr = np.asarray(arr)
                sort_cols.append((arr, desc))
            idx = np.arange(n_out)
            for arr, desc in sort_cols:
                a = arr[idx]
                o = np.argsort(a, kind="stable")
                if desc:
                    o = o[::-1]
                idx = idx[o]
            keep_idx = idx[keep[idx]]
        else:
            keep_idx = np.flatnonzero(keep)
        if plan.offset:
            keep_idx = keep_idx[plan.offset:]
        if plan.limit is not None:
            keep_idx = keep_idx[: plan.limit]
        cols = [c[keep_idx] for c in cols]
        return QueryResult(names, cols, kinds)

    # ------------------------------------------------------ RANGE queries

    _RANGE_MODES = {"min": 6, "max": 7, "sum": 5, "avg": 4, "mean": 4,
                    "count": 8, "last_value": 9, "__last_ts": 20}

    def _exec_range_select(self, sel: ast.Select, plan: SelectPlan) -> QueryResult:
        """SQL RANGE query: `agg(x) RANGE '10s' … ALIGN '5s' [TO …] [BY (…)]
        [FILL …]` — sliding window [t, t+range) per aligned step t
        (ref src/query/src/range_select/plan.rs:947: align_ts <= ts <
        align_ts + range). MI355X path: per-(group, field) NaN-compacted
        sample streams sorted by (slot, ts) feed the prom_range_eval window
        kernel with te = t + range - 1 (integer-ms shift turns the kernel's
        (tb, te] window into [t, t+range))."""
        from greptimedb_amd.ops import prom_range_eval
        st = plan.table
        device = self.engine.config.device
        schema = st.schema
        ts_name = schema.time_index.name
        if sel.align_ms is None:
            raise PlanQuery("RANGE queries need an ALIGN clause")
        align = sel.align_ms

        # collect RangeAgg nodes from the projections
        nodes: list[ast.RangeAgg] = []
        for e, _a in sel.projections:
            _collect_range_aggs(e, nodes)
        calls = []   # (node, func, field|None)
        for nd in nodes:
            f = nd.func
            fname = "avg" if f.name == "mean" else f.name
            if fname not in self._RANGE_MODES:
                raise PlanQuery(f"unsupported RANGE aggregate {f.name}")
            if len(f.args) == 1 and isinstance(f.args[0], ast.Star):
                arg = ts_name      # count(*): every row has a timestamp
            elif len(f.args) == 1 and isinstance(f.args[0], ast.Col):
                arg = f.args[0].name
            else:
                raise PlanQuery(f"RANGE aggregate needs a column arg: {f.name}")
            calls.append((nd, fname, arg))
        fields = sorted({arg for _nd, _f, arg in calls})
        col_fields = [fn for fn in fields if fn != ts_name]

        gt = sel.align_by if sel.align_by is not None else \
            [c.name for c in schema.tag_columns]
        group_keys, region_luts = self._build_group_luts(st, plan, gt)
        n_slots = max(len(group_keys), 1)

        ts_lo = plan.ts_lo if plan.ts_lo is not None else -(1 << 62)
        ts_hi = plan.ts_hi if plan.ts_hi is not None else (1 << 62)

        # gather per-field (slot, ts)-sorted sample streams (NaN compacted)
        parts = []          # (ts, slots, {field: vals})
        for region, lut in zip(st.regions, region_luts):
            self._cancel_check()
            lut_t = torch.as_tensor(lut, device=device)
            chunks = []
            for src in region.scan_sources(ts_lo, ts_hi):
                mask = filter_series_time(src.ts, src.series, lut_t, ts_lo, ts_hi)
                if plan.residual is not None:
                    mask &= self._eval_mask(plan.residual, src, region, device)
                idx = mask.nonzero(as_tuple=True)[0]
                if idx.numel() == 0:
                    continue
                fv = dict(zip(col_fields, src.take_fields(idx, col_fields)))
                if ts_name in fields:
                    fv[ts_name] = src.ts[idx].double()
                chunks.append((src.ts[idx], src.series[idx], fv))
            if not chunks:
                continue
            ts_t = torch.cat([c[0] for c in chunks])
            se_t = torch.cat([c[1] for c in chunks])
            fv = {fn: torch.cat([c[2][fn] for c in chunks]) for fn in fields}
            if not st.append_mode:   # last-wins dedup on (series, ts)
                p2 = sort_perm(se_t, ts_t)
                ts_t, se_t = ts_t[p2], se_t[p2]
                fv = {fn: v[p2] for fn, v in fv.items()}
                kidx = last_row_index(se_t, ts_t)
                if kidx.numel() != ts_t.numel():
                    ts_t, se_t = ts_t[kidx], se_t[kidx]
                    fv = {fn: v[kidx] for fn, v in fv.items()}
            sl_t = lut_t[se_t.long()]
            ok = sl_t >= 0
            if not bool(ok.all()):
                ts_t, sl_t = ts_t[ok], sl_t[ok]
                fv = {fn: v[ok] for fn, v in fv.items()}
            parts.append((ts_t, sl_t, fv))

        names_out, cols_out, kinds = [], [], []
        dist_ctx = self.dist
        if parts:
            ts_all = torch.cat([p[0] for p in parts])
            sl_all = torch.cat([p[1] for p in parts])
            perm = sort_perm(sl_all, ts_all)
            ts_all, sl_all = ts_all[perm], sl_all[perm]
            fvals = {fn: torch.cat([p[2][fn] for p in parts])[perm]
                     for fn in fields}
            data_lo, data_hi = int(ts_all.min()), int(ts_all.max())
        else:
            ts_all = torch.zeros(0, dtype=torch.int64, device=device)
            sl_all = torch.zeros(0, dtype=torch.int64, device=device)
            fvals = {fn: torch.zeros(0, dtype=torch.float64, device=device)
                     for fn in fields}
            data_lo = data_hi = None
        if dist_ctx is not None:
            data_lo, data_hi = dist_ctx.minmax_ts(data_lo, data_hi)
        if data_lo is None:
            for e, a in sel.projections:
                names_out.append(a or _expr_name(e))
                cols_out.append(np.array([]))
            return QueryResult(names_out, cols_out)

        # align grid over the GLOBAL data span (TO: epoch 0 | NOW | literal)
        to = 0
        if sel.align_to == "now":
            import time as _time
            to = int(_time.time() * 1000) % align
        elif sel.align_to not in (None, "calendar"):
            from greptimedb_amd.utils.timeutil import parse_ts_ms
            to = int(parse_ts_ms(sel.align_to)) % align
        max_range = max(nd.range_ms for nd, _f, _a in calls)
        t_first = -(-(data_lo - max_range + 1 - to) // align) * align + to
        t_last = ((data_hi - to) // align) * align + to
        T = int((t_last - t_first) // align) + 1
        if T > 4 << 20:
            raise PlanQuery(f"RANGE grid too large: {T} steps")

        def kernel_plane(fname, rng_ms, arg):
            """One [n_slots, T] partial plane on this rank's samples."""
            v = fvals[arg]
            valid = ~torch.isnan(v)
            if bool(valid.all()):
                tsf, slf, vf = ts_all, sl_all, v
            else:
                kidx = valid.nonzero(as_tuple=True)[0]
                tsf, slf, vf = ts_all[kidx], sl_all[kidx], v[kidx]
            counts = torch.bincount(slf.long(), minlength=n_slots)
            seg_hi = torch.cumsum(counts, 0)
            seg_lo = seg_hi - counts
            # te = t + range - 1 ⇒ kernel window (t-1, t+range-1] = [t, t+range)
            return prom_range_eval(
                tsf.contiguous(), vf.contiguous().double(), seg_lo.contiguous(),
                seg_hi.contiguous(), T, t_first + rng_ms - 1, align,
                rng_ms, 0, 0.0, self._RANGE_MODES[fname])

        planes: dict[int, np.ndarray] = {}
        if dist_ctx is None:
            for nd, fname, arg in calls:
                planes[id(nd)] = kernel_plane(fname, nd.range_ms, arg).cpu().numpy()
        else:
            # distributed: per-rank PRIMITIVE planes (sum/count/min/max),
            # group-unified + all-reduced, then finalized (avg = Σs/Σc).
            keys_sorted = [k for k, _s in sorted(group_keys.items(),
                                                 key=lambda kv: kv[1])]
            prim_specs: list = []       # (plane tensor [G, T], reduce op)
            call_prims: list = []       # per call: (kind, idx...) into outs
            last_pairs: list = []       # (ts_plane, val_plane) per last_value
            for nd, fname, arg in calls:
                G = len(keys_sorted)
                if fname == "last_value":
                    # argmax-by-timestamp merge: the newest sample across
                    # ranks wins (reference: final last_value at frontend)
                    ts_p = kernel_plane("__last_ts", nd.range_ms, arg)[:G]
                    v_p = kernel_plane("last_value", nd.range_ms, arg)[:G]
                    call_prims.append(("last", len(last_pairs)))
                    last_pairs.append((ts_p, v_p))
                    continue
                if fname in ("sum", "avg", "count"):
                    s_p = torch.nan_to_num(
                        kernel_plane("sum", nd.range_ms, arg), nan=0.0)[:G]
                    c_p = torch.nan_to_num(
                        kernel_plane("count", nd.range_ms, arg), nan=0.0)[:G]
                    call_prims.append((fname, len(prim_specs),
                                       len(prim_specs) + 1))
                    prim_specs += [(s_p, "sum"), (c_p, "sum")]
                else:   # min / max
                    p = kernel_plane(fname, nd.range_ms, arg)[:G]
                    fillv = float("inf") if fname == "min" else float("-inf")
                    p = torch.nan_to_num(p, nan=fillv, posinf=None, neginf=None)
                    call_prims.append((fname, len(prim_specs)))
                    prim_specs += [(p, fname)]
            merged_keys, outs = dist_ctx.merge_planes(keys_sorted, prim_specs)
            group_keys = {k: i for i, k in enumerate(merged_keys)}
            n_slots = max(len(group_keys), 1)
            for (nd, fname, arg), prim in zip(calls, call_prims):
                if prim[0] == "last":
                    ts_p, v_p = last_pairs[prim[1]]
                    _mk, plane_t = dist_ctx.argmax_combine(keys_sorted,
                                                           ts_p, v_p)
                    plane = plane_t.cpu().numpy()
                    if plane.shape[0] == 0:
                        plane = np.full((1, T), np.nan)
                    planes[id(nd)] = plane
                    continue
                if prim[0] in ("sum", "avg", "count"):
                    s = outs[prim[1]].cpu().numpy()
                    c = outs[prim[2]].cpu().numpy()
                    if fname == "count":
                        plane = np.where(c > 0, c, np.nan)
                    elif fname == "sum":
                        plane = np.where(c > 0, s, np.nan)
                    else:
                        plane = np.where(c > 0, s / np.where(c > 0, c, 1), np.nan)
                else:
                    p = outs[prim[1]].cpu().numpy()
                    plane = np.where(np.isfinite(p), p, np.nan)
                if plane.shape[0] == 0:
                    plane = np.full((1, T), np.nan)
                planes[id(nd)] = plane
        for nd, _fname, _arg in calls:
            fill = nd.fill if nd.fill is not None else sel.align_fill
            planes[id(nd)] = _apply_fill(planes[id(nd)], fill)

        grid = t_first + np.arange(T, dtype=np.int64) * align
        # drop rows where every RANGE column is NaN (reference emits only
        # align_ts slots that hold data unless FILL materializes them)
        any_fill = any((nd.fill if nd.fill is not None else sel.align_fill)
                       is not None for nd, _f, _a in calls)
        present = np.zeros((n_slots, T), dtype=bool)
        for p in planes.values():
            present |= ~np.isnan(p)
        if any_fill:
            rows_mask = present.any(axis=1)[:, None] & np.ones((1, T), dtype=bool)
        else:
            rows_mask = present
        slot_idx, t_idx = np.nonzero(rows_mask)
        # group-key columns
        keys_by_slot = [None] * n_slots
        for k, s in group_keys.items():
            keys_by_slot[s] = k
        col_data: dict[str, np.ndarray] = {ts_name: grid[t_idx]}
        for gi, g in enumerate(gt):
            per_slot = np.array([k[gi] if k else None for k in keys_by_slot],
                                dtype=object)
            col_data[g] = per_slot[slot_idx]
        for nid, p in planes.items():
            col_data[f"__range@{nid}"] = p[slot_idx, t_idx]

        # projections (RangeAgg nodes resolve via their precomputed planes)
        for e, a in sel.projections:
            name = a or _expr_name(e)
            names_out.append(name)
            kinds.append("ts" if isinstance(e, ast.Col) and e.name == ts_name else "")
            if isinstance(e, ast.Col):
                if e.name not in col_data:
                    raise PlanQuery(f"RANGE projection column {e.name} must be "
                                    f"the time index or an ALIGN BY column")
                cols_out.append(col_data[e.name])
            elif isinstance(e, ast.RangeAgg):
                cols_out.append(col_data[f"__range@{id(e)}"])
            elif isinstance(e, ast.Func) and e.name == "date_trunc":
                cols_out.append(col_data[ts_name])
            else:
                cols_out.append(np.asarray(_eval_np_expr(e, col_data)))

        r = QueryResult(names_out, cols_out, kinds)
        return _apply_order_limit(r, sel, names_out, default_order=[ts_name] + gt)

    def _exec_raw(self, sel: ast.Select, plan: SelectPlan) -> QueryResult:
        reservations: list = []
        try:
            return self._exec_raw_inner(sel, plan, reservations)
        finally:
            for r in reservations:
                r.release()

    def _exec_raw_inner(self, sel: ast.Select, plan: SelectPlan,
                        reservations: list) -> QueryResult:
        st = plan.table
        schema = st.schema
        device = self.engine.config.device
        ts_name = schema.time_index.name
        tag_names = [c.name for c in schema.tag_columns]
        field_names = st.regions[0].field_names
        str_field_names = []
        for region in st.regions:
            for sn in region.str_field_names:
                if sn not in str_field_names:
                    str_field_names.append(sn)

        # output columns; scalar expressions over fields/ts are computed
        # per-source on device (value() evaluator) into synthetic columns
        out_cols: list[str] = []
        expr_cols: list[tuple[str, ast.Expr]] = []
        for i, (e, alias) in enumerate(sel.projections):
            if isinstance(e, ast.Star):
                out_cols.extend(tag_names + [ts_name] + field_names + str_field_names)
            elif isinstance(e, ast.Col):
                if e.name != ts_name and e.name not in tag_names and \
                        e.name not in field_names and \
                        e.name not in str_field_names:
                    raise InvalidArguments(
                        f"unknown column {e.name!r} in table {st.schema.name}")
                out_cols.append(e.name)
            else:
                name = alias or _expr_name(e)
                expr_cols.append((name, e))
                out_cols.append(name)
        expr_names = {n for n, _ in expr_cols}
        needed_fields = [c for c in out_cols
                         if c in field_names and c not in expr_names]
        expr_ref: set = set()
        for _n, e in expr_cols:
            for c in _expr_cols(e):
                expr_ref.add(c)
                if c in field_names:
                    if c not in needed_fields:
                        needed_fields.append(c)
                elif c in tag_names or c == ts_name or c in str_field_names:
                    pass
                else:
                    raise PlanQuery(f"unknown column {c} in projection expr")
        needed_strs = [c for c in out_cols if c in str_field_names]
        for c in expr_ref:
            if c in str_field_names and c not in needed_strs:
                needed_strs.append(c)
        order_cols = [e.name for e, _ in plan.order_by if isinstance(e, ast.Col)]
        for c in order_cols:
            if c in field_names and c not in needed_fields:
                needed_fields.append(c)

        ts_lo = plan.ts_lo if plan.ts_lo is not None else -(1 << 62)
        ts_hi = plan.ts_hi if plan.ts_hi is not None else (1 << 62)

        # scan memory quota: reserve host bytes per materialized region part
        # (ref common/memory-manager scan pool); released when the result
        # is built
        row_bytes = 8 + 4 + 8 * max(len(needed_fields), 1) + \
            64 * len(needed_strs)
        parts = []  # (ts np, codes np, region, fields np [nf_needed, n])
        for region in st.regions:
            self._cancel_check()
            cand = self._candidate_codes(region, plan)
            lut = None
            if cand is not None:
                lut = np.full(len(region.series), -1, dtype=np.int32)
                lut[cand] = 1
            lut_t = torch.as_tensor(lut, device=device) if lut is not None else None
            chunks = []
            for src in region.scan_sources(ts_lo, ts_hi):
                mask = filter_series_time(src.ts, src.series, lut_t, ts_lo, ts_hi)
                if plan.residual is not None:
                    mask &= self._eval_mask(plan.residual, src, region, device)
                idx = mask.nonzero(as_tuple=True)[0]
                if idx.numel() == 0:
                    continue
                ts_t = src.ts[idx]
                se_t = src.series[idx]
                f_rows = src.take_fields(idx, needed_fields)
                f_t = torch.stack(f_rows) if f_rows else torch.zeros((0, idx.numel()), device=device)
                s_vals = {}
                if needed_strs:
                    hidx = idx.cpu().numpy()
                    for sn in needed_strs:
                        col = src.str_cols.get(sn)
                        if col is None:
                            s_vals[sn] = np.full(len(hidx), None, dtype=object)
                        else:
                            s_vals[sn] = np.asarray(col, dtype=object)[hidx]
                chunks.append((ts_t, se_t, f_t, s_vals))
            if not chunks:
                continue
            ts_t = torch.cat([c[0] for c in chunks])
            se_t = torch.cat([c[1] for c in chunks])
            f_t = torch.cat([c[2] for c in chunks], dim=1) if needed_fields else \
                torch.zeros((0, ts_t.numel()), device=device)
            s_cols = {sn: np.concatenate([c[3][sn] for c in chunks])
                      for sn in needed_strs}
            if not st.append_mode:
                # sort by (series, ts, arrival) then keep last
                ts_t, se_t, f_t, perm, kidx = sort_last_rows(se_t, ts_t, f_t)
                if needed_strs:
                    sel_h = perm[kidx].cpu().numpy()
                    s_cols = {sn: v[sel_h] for sn, v in s_cols.items()}
            reservations.append(
                self.engine.scan_quota.acquire(ts_t.numel() * row_bytes))
            parts.append((ts_t.cpu().numpy(), se_t.cpu().numpy(), region,
                          f_t.cpu().numpy(), s_cols))

        # materialize host rows (incl. columns referenced only inside
        # projection expressions, e.g. OVER (PARTITION BY tag ORDER BY ts))
        avail = set(tag_names) | {ts_name} | set(field_names) | set(str_field_names)
        mat_cols = (set(out_cols) | set(order_cols) | set(needed_fields) |
                    {ts_name} | (expr_ref & avail) if expr_cols
                    else set(out_cols) | set(order_cols))
        col_data = {c: [] for c in mat_cols if c not in expr_names}
        for ts_h, se_h, region, f_h, s_cols in parts:
            for c in col_data:
                if c == ts_name:
                    col_data[c].append(ts_h)
                elif c in tag_names:
                    col_data[c].append(region.series.tag_array(c)[se_h])
                elif c in needed_fields:
                    col_data[c].append(f_h[needed_fields.index(c)])
                elif c in needed_strs:
                    col_data[c].append(s_cols[c])
                else:
                    raise PlanQuery(f"unknown column {c}")
        if parts:
            col_data = {c: np.concatenate(v) for c, v in col_data.items()}
        else:
            col_data = {c: np.array([]) for c in col_data}
        if self.dist is not None:
            col_data = self.dist.gather_columns(col_data)
        n = len(next(iter(col_data.values()))) if col_data else 0
        # window functions first (they feed the projection expressions)
        win_nodes: list = []
        for _n2, e in expr_cols:
            _collect_window_nodes(e, win_nodes)
        for node in win_nodes:
            col_data[f"__win@{id(node)}"] = _compute_window(node, col_data, n) \
                if n else np.array([])
        # projection expressions over materialized columns (numpy)
        for name, e in expr_cols:
            if not n:
                col_data[name] = np.array([])
                continue
            a = np.asarray(_eval_np_expr(e, col_data))
            if a.ndim == 0:
                a = np.full(n, float(a))
            elif a.dtype != object and a.dtype.kind not in "US":
                a = a.astype(np.float64, copy=False)
            col_data[name] = a

        idx = np.arange(n)
        if sel.distinct and n:
            import pandas as pd
            df = pd.DataFrame({c: col_data[c] for c in out_cols})
            idx = df.drop_duplicates().index.to_numpy()
        for e, desc in reversed(plan.order_by):
            if not isinstance(e, ast.Col):
                raise PlanQuery("raw ORDER BY supports columns only")
            a = col_data[e.name][idx]
            o = np.argsort(a, kind="stable")
            if desc:
                o = o[::-1]
            idx = idx[o]
        if plan.offset:
            idx = idx[plan.offset:]
        if plan.limit is not None:
            idx = idx[: plan.limit]

        names, cols, kinds = [], [], []
        for c in out_cols:
            names.append(c)
            cols.append(col_data[c][idx])
            kinds.append("ts" if c == ts_name else "")
        return QueryResult(names, cols, kinds)

    # ------------------------------------------------------ predicate eval

    def _eval_mask(self, e: ast.Expr, src, region, device) -> torch.Tensor:
        """Vectorized residual-predicate evaluation over one scan source."""
        n = src.ts.numel()
        ts_name = region.schema.time_index.name
        tag_names = set(region.series.tag_names)

        def value(x):
            if isinstance(x, ast.Lit):
                return x.value
            if isinstance(x, ast.Col):
                if x.name == ts_name:
                    return src.ts
                p = src.field_pos.get(x.name)
                if p is not None:
                    return src.fields[p][:n]
                if x.name in tag_names:
                    return ("__tag__", x.name)
                if x.name in src.str_cols or x.name in region.str_field_names:
                    return ("__str__", x.name)
                raise PlanQuery(f"unknown column {x.name}")
            if isinstance(x, ast.UnaryOp) and x.op == "-":
                return -_as_t(value(x.operand))
            if isinstance(x, ast.BinOp) and x.op in ("+", "-", "*", "/", "%"):
                return _np_binop(x.op, _as_t(value(x.left)), _as_t(value(x.right)))
            if isinstance(x, ast.Interval):
                return x.ms
            if isinstance(x, ast.CorrMap):
                # decorrelated subquery: per-series threshold LUT (device)
                vals = region.series.tag_array(x.outer_col)
                arr = np.array([x.map.get(v, np.nan) for v in vals],
                               dtype=np.float64)
                if len(arr) == 0:
                    return torch.full((n,), float("nan"), device=device)
                lut = torch.as_tensor(arr, device=device)
                return lut[src.series.long()]
            if isinstance(x, ast.Func):
                return _eval_const(x)    # now() etc — constant-folded
            raise PlanQuery(f"unsupported predicate operand {x}")

        def _as_t(v):
            return v

        def tag_mask(tag, test) -> torch.Tensor:
            vals = region.series.tag_array(tag)
            codes_ok = np.array([bool(test(v)) for v in vals], dtype=bool)
            lut = torch.as_tensor(codes_ok, device=device)
            if len(codes_ok) == 0:
                return torch.zeros(n, dtype=torch.bool, device=device)
            return lut[src.series.long()]

        def ev(x) -> torch.Tensor:
            if isinstance(x, ast.Func) and x.name in ("matches", "matches_term"):
                # fulltext probe (reference: matches/matches_term UDFs over the
                # tantivy index; here: GPU posting-list probe, engine/fulltext.py)
                if len(x.args) != 2 or not isinstance(x.args[0], ast.Col) or \
                        not isinstance(x.args[1], ast.Lit):
                    raise PlanQuery("matches(column, 'query') expected")
                col = x.args[0].name
                q = str(x.args[1].value)
                import re as _re2
                terms = _re2.findall(r"[A-Za-z0-9]+", q.lower())
                if not terms:
                    return torch.ones(n, dtype=torch.bool, device=device)
                if src.text_probe is None:
                    raise PlanQuery(f"no fulltext index on column {col}")
                m = src.text_probe(col, terms)
                if m is None:
                    raise PlanQuery(f"no fulltext index on column {col}")
                return m
            if isinstance(x, ast.BinOp):
                if x.op == "and":
                    return ev(x.left) & ev(x.right)
                if x.op == "or":
                    return ev(x.left) | ev(x.right)
                if x.op in ("=", "!=", "<>", "<", "<=", ">", ">="):
                    lv, rv = value(x.left), value(x.right)
                    # string-field comparison → host column eval
                    if isinstance(lv, tuple) and lv[0] == "__str__":
                        col = src.str_cols.get(lv[1])
                        if col is None:
                            return torch.zeros(n, dtype=torch.bool, device=device)
                        arr = np.asarray(col, dtype=object)
                        res = np.array([_py_cmp(x.op, v, rv) for v in arr], dtype=bool)
                        return torch.as_tensor(res, device=device)
                    # tag comparison → host-side per-code eval
                    if isinstance(lv, tuple) and lv[0] == "__tag__":
                        tag = lv[1]
                        rr = rv
                        op = x.op
                        return tag_mask(tag, lambda v: _py_cmp(op, v, rr))
                    if isinstance(rv, tuple) and rv[0] == "__tag__":
                        tag = rv[1]
                        ll = lv
                        op = x.op
                        return tag_mask(tag, lambda v: _py_cmp(op, ll, v))
                    lt = lv if torch.is_tensor(lv) else None
                    rt = rv if torch.is_tensor(rv) else None
                    if lt is None and rt is None:
                        return torch.full((n,), bool(_py_cmp(x.op, lv, rv)),
                                          dtype=torch.bool, device=device)
                    # coerce ts string literals
                    if lt is src.ts and isinstance(rv, str):
                        rv = _lit_ts_ms(rv, True)
                    if rt is src.ts and isinstance(lv, str):
                        lv = _lit_ts_ms(lv, True)
                    l = lv if torch.is_tensor(lv) else float(lv)
                    r = rv if torch.is_tensor(rv) else float(rv)
                    return _torch_cmp(x.op, l, r)
                if x.op == "like":
                    lv = value(x.left)
                    import fnmatch
                    raw = str(value(x.right))
                    # honor \% and \_ escapes (log-query Contains quoting)
                    pat = (raw.replace(r"\%", "\x00").replace(r"\_", "\x01")
                              .replace("%", "*").replace("_", "?")
                              .replace("\x00", "%").replace("\x01", "_"))
                    if isinstance(lv, tuple) and lv[0] == "__tag__":
                        return tag_mask(lv[1], lambda v: v is not None and
                                        fnmatch.fnmatch(v, pat))
                    if isinstance(lv, tuple) and lv[0] == "__str__":
                        col = src.str_cols.get(lv[1])
                        if col is None:
                            return torch.zeros(n, dtype=torch.bool, device=device)
                        res = np.array([v is not None and
                                        fnmatch.fnmatch(str(v), pat)
                                        for v in col], dtype=bool)
                        return torch.as_tensor(res, device=device)
                    raise PlanQuery("LIKE only on string columns")
            if isinstance(x, ast.UnaryOp) and x.op == "not":
                return ~ev(x.operand)
            if isinstance(x, ast.InList):
                lv = value(x.expr)
                items = [value(i) for i in x.items]
                if isinstance(lv, tuple) and lv[0] == "__tag__":
                    s = set(map(str, items))
                    m = tag_mask(lv[1], lambda v: v in s)
                else:
                    m = torch.zeros(n, dtype=torch.bool, device=device)
                    for it in items:
                        m |= _torch_cmp("=", lv, float(it))
                return ~m if x.negated else m
            if isinstance(x, ast.Between):
                lo = ev(ast.BinOp(">=", x.expr, x.low))
                hi = ev(ast.BinOp("<=", x.expr, x.high))
                m = lo & hi
                return ~m if x.negated else m
            if isinstance(x, ast.IsNull):
                lv = value(x.expr)
                if torch.is_tensor(lv) and lv.dtype == torch.float64:
                    m = torch.isnan(lv)
                elif isinstance(lv, tuple) and lv[0] == "__tag__":
                    m = tag_mask(lv[1], lambda v: v is None)
                else:
                    m = torch.zeros(n, dtype=torch.bool, device=device)
                return ~m if x.negated else m
            if isinstance(x, ast.Lit):
                return torch.full((n,), bool(x.value), dtype=torch.bool, device=device)
            raise PlanQuery(f"unsupported predicate {x}")

        return ev(e)


# ------------------------------------------------------------------ helpers


def _py_cmp(op, a, b):
    if a is None or b is None:
        return False
    try:
        if op == "=":
            return a == b
        if op in ("!=", "<>"):
            return a != b
        if op == "<":
            return a < b
        if op == "<=":
            return a <= b
        if op == ">":
            return a > b
        if op == ">=":
            return a >= b
    except TypeError:
        return False
    raise PlanQuery(f"cmp {op}")


def _torch_cmp(op, a, b):
    if op == "=":
        return a == b
    if op in ("!=", "<>"):
        return a != b
    if op == "<":
        return a < b
    if op == "<=":
        return a <= b
    if op == ">":
        return a > b
    if op == ">=":
        return a >= b
    raise PlanQuery(f"cmp {op}")


def _np_binop(op, l, r):
    if op == "+":
        return l + r
    if op == "-":
        return l - r
    if op == "*":
        return l * r
    if op == "/":
        return l / r
    if op == "%":
        return l % r
    if op == "=":
        return l == r
    if op in ("!=", "<>"):
        return l != r
    if op == "<":
        return l < r
    if op == "<=":
        return l <= r
    if op == ">":
        return l > r
    if op == ">=":
        return l >= r
    if op == "and":
        return np.asarray(l, dtype=bool) & np.asarray(r, dtype=bool)
    if op == "or":
        return np.asarray(l, dtype=bool) | np.asarray(r, dtype=bool)
    raise PlanQuery(f"binop {op}")


_NP_FUNCS = {"abs": np.abs, "floor": np.floor, "ceil": np.ceil,
             "sqrt": np.sqrt, "ln": np.log, "log2": np.log2,
             "log10": np.log10, "exp": np.exp}


# ---------------- object-typed scalar UDFs (json / geo / string / vector) ---
# ref: src/common/function/src/scalars/{json,geo,vector} — the practical
# subset; each takes raw (object) numpy columns and is vectorized in python.

def _json_path_norm(path: str) -> str:
    p = str(path)
    if p.startswith("$"):
        p = p[1:]
    if p and not p.startswith((".", "[")):
        p = "." + p
    return p


def _json_get(col, path, conv):
    import json as _json
    from greptimedb_amd.pipeline.engine import _json_path_get
    p = _json_path_norm(path)
    out = np.empty(len(col), dtype=object)
    for i, s in enumerate(col):
        v = None
        if s is not None:
            try:
                v = _json_path_get(_json.loads(s) if isinstance(s, str) else s,
                                   "$" + p)
            except (ValueError, TypeError):
                v = None
        out[i] = conv(v)
    return out


def _to_num(arr):
    return np.array([np.nan if v is None else float(v) for v in arr])


def _haversine_m(lat1, lng1, lat2, lng2):
    r = 6371008.8
    p1, p2 = np.radians(lat1), np.radians(lat2)
    dp = p2 - p1
    dl = np.radians(lng2) - np.radians(lng1)
    a = np.sin(dp / 2) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(dl / 2) ** 2
    return 2 * r * np.arcsin(np.sqrt(a))


_GEOHASH32 = "0123456789bcdefghjkmnpqrstuvwxyz"


def _geohash(lat, lng, precision):
    out = np.empty(len(np.atleast_1d(lat)), dtype=object)
    lat = np.atleast_1d(lat)
    lng = np.atleast_1d(lng)
    for i in range(len(out)):
        la, lo = float(lat[i]), float(lng[i % len(lng)] if len(lng) > 1 else lng[0])
        lat_r, lng_r = [-90.0, 90.0], [-180.0, 180.0]
        bits = []
        even = True
        while len(bits) < precision * 5:
            rng = lng_r if even else lat_r
            v = lo if even else la
            mid = (rng[0] + rng[1]) / 2
            if v >= mid:
                bits.append(1)
                rng[0] = mid
            else:
                bits.append(0)
                rng[1] = mid
            even = not even
        s = ""
        for c in range(precision):
            idx = 0
            for b in bits[c * 5:(c + 1) * 5]:
                idx = (idx << 1) | b
            s += _GEOHASH32[idx]
        out[i] = s
    return out


def _vec_decode(col):
    return [None if v is None else np.frombuffer(
        v if isinstance(v, (bytes, bytearray)) else str(v).encode("latin1"),
        dtype=np.float32) for v in col]


def _str_col(a, n=None):
    arr = np.atleast_1d(np.asarray(a, dtype=object))
    if n is not None and len(arr) == 1 and n > 1:
        arr = np.full(n, arr[0], dtype=object)
    return arr


_OBJ_FUNCS = {
    "json_get_string": lambda a: _json_get(
        _str_col(a[0]), a[1], lambda v: None if v is None else str(v)),
    "json_get_int": lambda a: _to_num(_json_get(
        _str_col(a[0]), a[1],
        lambda v: None if v is None or isinstance(v, (dict, list)) else int(float(v)))),
    "json_get_float": lambda a: _to_num(_json_get(
        _str_col(a[0]), a[1],
        lambda v: None if v is None or isinstance(v, (dict, list)) else float(v))),
    "json_get_bool": lambda a: _to_num(_json_get(
        _str_col(a[0]), a[1],
        lambda v: None if not isinstance(v, bool) else float(v))),
    "json_path_exists": lambda a: _to_num(_json_get(
        _str_col(a[0]), a[1], lambda v: float(v is not None))),
    "st_distance": lambda a: _haversine_m(_to_num_b(a[0]), _to_num_b(a[1]),
                                          _to_num_b(a[2]), _to_num_b(a[3])),
    "geohash": lambda a: _geohash(_to_num_b(a[0]), _to_num_b(a[1]),
                                  int(np.atleast_1d(a[2])[0])),
    "upper": lambda a: np.array([None if v is None else str(v).upper()
                                 for v in _str_col(a[0])], dtype=object),
    "lower": lambda a: np.array([None if v is None else str(v).lower()
                                 for v in _str_col(a[0])], dtype=object),
    "trim": lambda a: np.array([None if v is None else str(v).strip()
                                for v in _str_col(a[0])], dtype=object),
    "length": lambda a: np.array([np.nan if v is None else float(len(str(v)))
                                  for v in _str_col(a[0])]),
    # substr(s, start_1based[, len]) — SQL semantics (reference DataFusion)
    "substr": lambda a: np.array(
        [None if v is None else
         str(v)[max(int(np.atleast_1d(a[1])[0]) - 1, 0):
                (max(int(np.atleast_1d(a[1])[0]) - 1, 0) +
                 int(np.atleast_1d(a[2])[0])) if len(a) > 2 else None]
         for v in _str_col(a[0])], dtype=object),
    "char_length": lambda a: _OBJ_FUNCS["length"](a),
    "replace": lambda a: np.array(
        [None if v is None else str(v).replace(str(np.atleast_1d(a[1])[0]),
                                               str(np.atleast_1d(a[2])[0]))
         for v in _str_col(a[0])], dtype=object),
    "concat": lambda a: _concat_cols(a),
    "vec_dim": lambda a: np.array(
        [np.nan if v is None else float(len(v)) for v in _vec_decode(_str_col(a[0]))]),
    "vec_to_string": lambda a: np.array(
        ["[" + ",".join(f"{x:g}" for x in v) + "]" if v is not None else None
         for v in _vec_decode(_str_col(a[0]))], dtype=object),
    "coalesce": lambda a: _coalesce(a),
    "nullif": lambda a: _nullif(a),
    "greatest": lambda a: __import__("functools").reduce(
        np.fmax, [_to_num_b(x) for x in a]),
    "least": lambda a: __import__("functools").reduce(
        np.fmin, [_to_num_b(x) for x in a]),
}


def _coalesce(args):
    cols = [np.atleast_1d(np.asarray(a, dtype=object)) for a in args]
    n = max(len(c) for c in cols)
    cols = [np.full(n, c[0], dtype=object) if len(c) == 1 and n > 1 else c
            for c in cols]
    out = np.full(n, None, dtype=object)
    for c in cols:
        need = np.array([v is None or (isinstance(v, float) and np.isnan(v))
                         for v in out])
        out[need] = c[need]
    return out


def _nullif(args):
    a = np.atleast_1d(np.asarray(args[0], dtype=object))
    b = args[1]
    bv = np.atleast_1d(np.asarray(b, dtype=object))
    if len(bv) == 1 and len(a) > 1:
        bv = np.full(len(a), bv[0], dtype=object)
    out = a.copy()
    out[a == bv] = None
    return out


def _to_num_b(a):
    arr = np.atleast_1d(np.asarray(a))
    if arr.dtype == object:
        return _to_num(arr)
    return arr.astype(np.float64)


def _concat_cols(args):
    cols = [np.atleast_1d(np.asarray(a, dtype=object)) for a in args]
    n = max(len(c) for c in cols)
    cols = [np.full(n, c[0], dtype=object) if len(c) == 1 and n > 1 else c
            for c in cols]
    return np.array(["".join("" if c[i] is None else str(c[i]) for c in cols)
                     for i in range(n)], dtype=object)


def _np_raw(e: ast.Expr, col_data: dict):
    """Like _eval_np_expr but keeps object (string) columns unconverted."""
    if isinstance(e, ast.Col):
        return np.asarray(col_data[e.name])
    if isinstance(e, ast.Lit):
        return e.value
    return _eval_np_expr(e, col_data)


def _np_isnull(v) -> np.ndarray:
    a = np.asarray(v)
    if a.dtype == object:
        return np.array([x is None or (isinstance(x, float) and np.isnan(x))
                         for x in a], dtype=bool)
    return np.isnan(a.astype(np.float64))


def _eval_np_cond(e: ast.Expr, col_data: dict) -> np.ndarray:
    """Boolean predicate over materialized columns (CASE WHEN conditions) —
    comparisons stay raw so string/tag columns compare correctly."""
    if isinstance(e, ast.BinOp) and e.op in ("=", "!=", "<>", "<", "<=",
                                             ">", ">="):
        return np.asarray(_np_binop(e.op, _np_raw(e.left, col_data),
                                    _np_raw(e.right, col_data)), dtype=bool)
    if isinstance(e, ast.BinOp) and e.op in ("and", "or"):
        return _np_binop(e.op, _eval_np_cond(e.left, col_data),
                         _eval_np_cond(e.right, col_data))
    if isinstance(e, ast.UnaryOp) and e.op == "not":
        return ~_eval_np_cond(e.operand, col_data)
    if isinstance(e, ast.IsNull):
        m = _np_isnull(_np_raw(e.expr, col_data))
        return ~m if e.negated else m
    if isinstance(e, ast.InList):
        v = _np_raw(e.expr, col_data)
        m = np.zeros(len(np.atleast_1d(v)), dtype=bool)
        for it in e.items:
            m |= np.asarray(np.atleast_1d(v) == _np_raw(it, col_data),
                            dtype=bool)
        return ~m if e.negated else m
    return np.asarray(_eval_np_expr(e, col_data), dtype=bool)


def _eval_np_expr(e: ast.Expr, col_data: dict):
    """Scalar expression over materialized numpy columns (raw-path
    projections like `v * 8 / 1024`)."""
    if isinstance(e, ast.WindowFunc):
        return col_data[f"__win@{id(e)}"]  # precomputed by _compute_window
    if isinstance(e, ast.RangeAgg):
        return col_data[f"__range@{id(e)}"]  # precomputed range plane slice
    if isinstance(e, ast.Col):
        return np.asarray(col_data[e.name], dtype=np.float64)
    if isinstance(e, ast.Lit):
        return float(e.value)
    if isinstance(e, ast.BinOp):
        return _np_binop(e.op, _eval_np_expr(e.left, col_data),
                         _eval_np_expr(e.right, col_data))
    if isinstance(e, ast.UnaryOp) and e.op == "-":
        return -_eval_np_expr(e.operand, col_data)
    if isinstance(e, ast.Cast):
        return _apply_cast(_np_raw(e.expr, col_data), e.type)
    if isinstance(e, ast.Case):
        conds, vals = [], []
        for w, r in e.whens:
            if e.operand is not None:
                c = np.asarray(np.atleast_1d(_np_raw(e.operand, col_data)) ==
                               _np_raw(w, col_data), dtype=bool)
            else:
                c = _eval_np_cond(w, col_data)
            conds.append(np.atleast_1d(c))
            vals.append(_np_raw(r, col_data))
        dflt = _np_raw(e.default, col_data) if e.default is not None else None
        n_rows = len(conds[0]) if conds else 0
        is_str = any(isinstance(v, str) or
                     (isinstance(v, np.ndarray) and v.dtype.kind in "OUS")
                     for v in vals + [dflt])
        if is_str:
            out = np.full(n_rows, dflt if np.ndim(dflt) == 0 else None,
                          dtype=object)
        else:
            out = np.full(n_rows, np.nan if dflt is None else dflt,
                          dtype=np.float64)
        if np.ndim(dflt) == 1:
            out[:] = dflt
        for c, v in reversed(list(zip(conds, vals))):   # first match wins
            if np.ndim(v) == 0:
                out[c] = v
            else:
                out[c] = np.asarray(v, dtype=out.dtype)[c]
        return out
    if isinstance(e, ast.Func) and e.name in _OBJ_FUNCS:
        return _OBJ_FUNCS[e.name]([_np_raw(a, col_data) for a in e.args])
    if isinstance(e, ast.Func) and e.name in _NP_FUNCS:
        return _NP_FUNCS[e.name](_eval_np_expr(e.args[0], col_data))
    if isinstance(e, ast.Func) and e.name == "round":
        v = _eval_np_expr(e.args[0], col_data)
        nd = int(e.args[1].value) if len(e.args) > 1 else 0
        return np.round(v, nd)
    raise PlanQuery(f"unsupported projection expr {e}")


def _has_subquery(e) -> bool:
    if e is None:
        return False
    if isinstance(e, (ast.ScalarSubquery, ast.Exists)):
        return True
    if isinstance(e, ast.BinOp):
        return _has_subquery(e.left) or _has_subquery(e.right)
    if isinstance(e, ast.UnaryOp):
        return _has_subquery(e.operand)
    if isinstance(e, ast.Func):
        return any(_has_subquery(a) for a in e.args)
    if isinstance(e, ast.Between):
        return _has_subquery(e.low) or _has_subquery(e.high)
    if isinstance(e, ast.InList):
        return any(_has_subquery(a) for a in e.items)
    return False


def _has_range_agg(e) -> bool:
    found: list = []
    _collect_range_aggs(e, found)
    return bool(found)


def _collect_range_aggs(e, out: list):
    if isinstance(e, ast.RangeAgg):
        out.append(e)
    elif isinstance(e, ast.BinOp):
        _collect_range_aggs(e.left, out)
        _collect_range_aggs(e.right, out)
    elif isinstance(e, ast.UnaryOp):
        _collect_range_aggs(e.operand, out)
    elif isinstance(e, ast.Func):
        for a in e.args:
            _collect_range_aggs(a, out)


def _apply_fill(plane: np.ndarray, fill) -> np.ndarray:
    """FILL NULL|PREV|LINEAR|<const> over an [S, T] range plane."""
    if fill is None or fill == "null":
        return plane
    if isinstance(fill, (int, float)) and not isinstance(fill, bool):
        return np.where(np.isnan(plane), float(fill), plane)
    S, T = plane.shape
    if fill == "prev":
        idx = np.where(~np.isnan(plane), np.arange(T)[None, :], 0)
        idx = np.maximum.accumulate(idx, axis=1)
        out = plane[np.arange(S)[:, None], idx]
        # positions before the first sample stay NaN
        first = np.argmax(~np.isnan(plane), axis=1)
        none = ~np.isnan(plane).any(axis=1)
        mask_before = np.arange(T)[None, :] < first[:, None]
        out[mask_before | none[:, None]] = np.nan
        return out
    if fill == "linear":
        out = plane.copy()
        x = np.arange(T, dtype=np.float64)
        for s in range(S):
            row = out[s]
            good = ~np.isnan(row)
            if good.sum() >= 2:
                out[s] = np.interp(x, x[good], row[good])
                # do not extrapolate beyond known points
                lo, hi = np.flatnonzero(good)[[0, -1]]
                out[s, :lo] = np.nan
                out[s, hi + 1:] = np.nan
        return out
    raise PlanQuery(f"unsupported FILL {fill!r}")


def _apply_order_limit(r: QueryResult, sel: ast.Select, names: list[str],
                       default_order: list[str]) -> QueryResult:
    """ORDER BY named output columns + LIMIT/OFFSET over a QueryResult."""
    n = len(r.columns[0]) if r.columns else 0
    idx = np.arange(n)
    order = sel.order_by or [(ast.Col(c), False) for c in default_order
                             if c in names]
    for e, desc in reversed(order):
        if not isinstance(e, ast.Col) or e.name not in names:
            continue
        a = np.asarray(r.columns[names.index(e.name)])[idx]
        if a.dtype == object or a.dtype.kind in "US":
            # factorize strings to dense codes: numpy sorts i64 codes ~7x
            # faster than python-object comparisons at 100k+ rows
            import pandas as pd
            codes, uniq = pd.factorize(a.astype(object), sort=True)
            a = codes.astype(np.int64)
        o = np.argsort(a, kind="stable")
        if desc:
            o = o[::-1]
        idx = idx[o]
    if sel.offset:
        idx = idx[sel.offset:]
    if sel.limit is not None:
        idx = idx[: sel.limit]
    return QueryResult(names, [np.asarray(c)[idx] for c in r.columns], r.kinds)


def _collect_window_nodes(e, out: list):
    if isinstance(e, ast.WindowFunc):
        out.append(e)
    elif isinstance(e, ast.BinOp):
        _collect_window_nodes(e.left, out)
        _collect_window_nodes(e.right, out)
    elif isinstance(e, ast.UnaryOp):
        _collect_window_nodes(e.operand, out)
    elif isinstance(e, ast.Func):
        for a in e.args:
            _collect_window_nodes(a, out)


def _win_sort_key(a: np.ndarray, desc: bool = False) -> np.ndarray:
    """lexsort-able key: strings factorized to dense codes, desc negated."""
    a = np.asarray(a)
    if a.dtype == object or a.dtype.kind in "US":
        _, inv = np.unique(a.astype(str), return_inverse=True)
        a = inv.astype(np.int64)
    return -a if desc else a


def _peer_ends(new_peer: np.ndarray, n: int) -> np.ndarray:
    """For each (sorted) row, the index of the LAST row of its peer group."""
    grp = np.cumsum(new_peer) - 1
    starts = np.flatnonzero(new_peer)
    return (np.append(starts[1:], n) - 1)[grp]


def _compute_window(node: "ast.WindowFunc", col_data: dict, n: int) -> np.ndarray:
    """Evaluate one window function over the materialized raw result
    (numpy, vectorized; ref: DataFusion WindowAggExec semantics with the
    default frame — running to the current row's peer group when ORDER BY
    is present, whole partition otherwise). Returns values in the
    ORIGINAL row order."""
    if n == 0:
        return np.array([])

    def raw(e):
        if isinstance(e, ast.Col):
            return np.asarray(col_data[e.name])
        return np.asarray(_eval_np_expr(e, col_data))

    keys = [_win_sort_key(raw(e2), desc) for e2, desc in reversed(node.order_by)]
    part_codes = [_win_sort_key(raw(e2)) for e2 in node.partition_by]
    perm = np.lexsort(tuple(keys) + tuple(part_codes)) if (keys or part_codes) \
        else np.arange(n)
    pos = np.arange(n)
    new_part = np.zeros(n, dtype=bool)
    new_part[0] = True
    for k in part_codes:
        ks = k[perm]
        new_part[1:] |= ks[1:] != ks[:-1]
    starts = np.flatnonzero(new_part)
    seg_id = np.cumsum(new_part) - 1
    start_of = starts[seg_id]
    new_peer = new_part.copy()
    for k in keys:
        ks = k[perm]
        new_peer[1:] |= ks[1:] != ks[:-1]

    name = "avg" if node.name == "mean" else node.name
    if name == "row_number":
        out_sorted = (pos - start_of + 1).astype(np.float64)
    elif name in ("rank", "dense_rank"):
        if name == "rank":
            peer_start = np.maximum.accumulate(np.where(new_peer, pos, 0))
            out_sorted = (peer_start - start_of + 1).astype(np.float64)
        else:
            d = np.cumsum(new_peer)
            out_sorted = (d - d[start_of] + 1).astype(np.float64)
    elif name in ("lag", "lead"):
        x = raw(node.args[0])[perm]
        k = int(_eval_const(node.args[1])) if len(node.args) > 1 else 1
        default = _eval_const(node.args[2]) if len(node.args) > 2 else None
        if name == "lead":
            k = -k
        is_obj = x.dtype == object
        out_sorted = np.empty(n, dtype=object if is_obj else np.float64)
        out_sorted[:] = default if is_obj else \
            (np.nan if default is None else float(default))
        if k != 0:
            src = np.clip(pos - k, 0, n - 1)
            ok = ((pos - k >= 0) & (pos - k < n)) & (seg_id[src] == seg_id)
            out_sorted[ok] = x[src[ok]]
        else:
            out_sorted = x if is_obj else x.astype(np.float64)
    elif name in ("first_value", "last_value"):
        x = raw(node.args[0])[perm]
        if name == "first_value":
            out_sorted = x[start_of]
        elif not node.order_by:               # whole partition → partition end
            out_sorted = x[np.append(starts[1:], n)[seg_id] - 1]
        else:                                 # default frame → peer-group end
            out_sorted = x[_peer_ends(new_peer, n)]
    elif name in ("sum", "avg", "min", "max", "count"):
        if not node.args or isinstance(node.args[0], ast.Star):
            x = np.ones(n, dtype=np.float64)
        else:
            x = np.asarray(raw(node.args[0]), dtype=np.float64)[perm]
        valid = ~np.isnan(x)
        if not node.order_by:  # whole-partition aggregate
            c = np.add.reduceat(valid.astype(np.float64), starts)
            if name in ("sum", "avg", "count"):
                s = np.add.reduceat(np.where(valid, x, 0.0), starts)
                v = c if name == "count" else \
                    (s if name == "sum" else s / np.where(c > 0, c, np.nan))
            else:
                xx = np.where(valid, x, np.inf if name == "min" else -np.inf)
                red = np.minimum if name == "min" else np.maximum
                v = np.where(c > 0, red.reduceat(xx, starts), np.nan)
            if name != "count":
                v = np.where(c > 0, v, np.nan)
            out_sorted = v[seg_id]
        else:  # running to the end of the current peer group
            pe = _peer_ends(new_peer, n)
            cc = np.cumsum(valid.astype(np.float64))
            base_c = np.where(start_of > 0, cc[np.maximum(start_of - 1, 0)], 0.0)
            c = cc[pe] - base_c
            if name in ("sum", "avg", "count"):
                cs = np.cumsum(np.where(valid, x, 0.0))
                base_s = np.where(start_of > 0, cs[np.maximum(start_of - 1, 0)], 0.0)
                s = cs[pe] - base_s
                v = c if name == "count" else \
                    (s if name == "sum" else s / np.where(c > 0, c, np.nan))
            else:
                xx = np.where(valid, x, np.inf if name == "min" else -np.inf)
                accf = np.minimum.accumulate if name == "min" else np.maximum.accumulate
                acc = np.empty(n, dtype=np.float64)
                for s0, s1 in zip(starts, np.append(starts[1:], n)):
                    acc[s0:s1] = accf(xx[s0:s1])
                v = acc[pe]
            out_sorted = np.where(c > 0, v, np.nan) if name != "count" else v
    else:
        raise PlanQuery(f"unsupported window function {node.name}")

    out = np.empty(n, dtype=out_sorted.dtype)
    out[perm] = out_sorted
    return out


def _eval_const(e: ast.Expr):
    if isinstance(e, ast.Lit):
        return e.value
    if isinstance(e, ast.Interval):
        return e.ms
    if isinstance(e, ast.BinOp):
        return _np_binop(e.op, _eval_const(e.left), _eval_const(e.right))
    if isinstance(e, ast.UnaryOp) and e.op == "-":
        return -_eval_const(e.operand)
    if isinstance(e, ast.Func) and e.name == "now":
        import time
        return int(time.time() * 1000)
    if isinstance(e, ast.Func):
        import math as _math
        one = {"abs": abs, "sqrt": _math.sqrt, "floor": _math.floor,
               "ceil": _math.ceil, "exp": _math.exp, "ln": _math.log,
               "log": _math.log10, "log2": _math.log2, "sin": _math.sin,
               "cos": _math.cos, "tan": _math.tan}
        fn = e.name.lower()
        if fn in one and len(e.args) == 1:
            return one[fn](float(_eval_const(e.args[0])))
        if fn in ("pow", "power") and len(e.args) == 2:
            return float(_eval_const(e.args[0])) ** float(_eval_const(e.args[1]))
        if fn == "round":
            nd = int(_eval_const(e.args[1])) if len(e.args) > 1 else 0
            return round(float(_eval_const(e.args[0])), nd)
        if fn in _OBJ_FUNCS:
            return _scalarize(_OBJ_FUNCS[fn](
                [np.atleast_1d(np.asarray(_eval_const(a), dtype=object))
                 for a in e.args]))
    if isinstance(e, ast.Cast):
        return _scalarize(_apply_cast(
            np.atleast_1d(np.asarray(_eval_const(e.expr), dtype=object)),
            e.type))
    if isinstance(e, ast.Case):
        for w, then in e.whens:
            cond = (_eval_const(e.operand) == _eval_const(w)) \
                if e.operand is not None else _eval_const(w)
            if cond:
                return _eval_const(then)
        return _eval_const(e.default) if e.default is not None else None
    raise PlanQuery(f"unsupported constant expr {e}")


def _scalarize(v):
    a = np.asarray(v)
    return a.item() if a.ndim == 0 or a.size == 1 else v


def _fold_const_casts(e):
    """Fold CAST over a constant subtree to a literal so WHERE time-bound /
    tag analysis sees plain literals (DataFusion constant folding)."""
    if isinstance(e, ast.Cast):
        if not _expr_cols(e.expr):
            try:
                return ast.Lit(_eval_const(e))
            except Exception:
                return e
        return ast.Cast(_fold_const_casts(e.expr), e.type)
    if isinstance(e, ast.BinOp):
        return ast.BinOp(e.op, _fold_const_casts(e.left),
                         _fold_const_casts(e.right))
    if isinstance(e, ast.UnaryOp):
        return ast.UnaryOp(e.op, _fold_const_casts(e.operand))
    if isinstance(e, ast.Between):
        return ast.Between(_fold_const_casts(e.expr),
                           _fold_const_casts(e.low),
                           _fold_const_casts(e.high), e.negated)
    return e


def _apply_cast(v, ty: str):
    """CAST semantics over a numpy column (reference: Arrow cast kernels)."""
    a = np.asarray(v)
    if ty in ("bigint", "int", "integer", "smallint", "tinyint",
              "int64", "int32", "uint64", "uint32"):
        f = a.astype(np.float64) if a.dtype != object else np.array(
            [np.nan if x is None else float(x) for x in a.ravel()]
        ).reshape(a.shape)
        out = np.where(np.isnan(f), np.nan, np.trunc(f))
        return out.astype(np.int64) if not np.isnan(out).any() else out
    if ty in ("double", "float", "real", "float64", "float32", "decimal"):
        if a.dtype == object:
            return np.array([np.nan if x is None else float(x)
                             for x in a.ravel()]).reshape(a.shape)
        return a.astype(np.float64)
    if ty in ("string", "text", "varchar", "char"):
        def s_of(x):
            if x is None:
                return None
            if isinstance(x, (float, np.floating)):
                return f"{float(x):g}"
            if isinstance(x, (int, np.integer)):
                return str(int(x))
            return str(x)
        return np.array([s_of(x) for x in a.ravel()],
                        dtype=object).reshape(a.shape)
    if ty in ("timestamp", "datetime"):
        from greptimedb_amd.utils.timeutil import parse_ts_ms as _p
        def t_of(x):
            if x is None:
                return np.nan
            if isinstance(x, str):
                ms = _p(x)
                if ms is None:
                    raise InvalidArguments(f"bad timestamp literal {x!r}")
                return float(ms)
            return float(x)
        return np.array([t_of(x) for x in a.ravel()],
                        dtype=np.float64).reshape(a.shape)
    if ty in ("boolean", "bool"):
        return np.array([None if x is None else bool(x) for x in a.ravel()],
                        dtype=object).reshape(a.shape)
    raise InvalidArguments(f"unsupported cast type {ty!r}")


def _expr_name(e: ast.Expr) -> str:
    if isinstance(e, ast.RangeAgg):
        return f"{_expr_name(e.func)} RANGE {e.range_ms}ms"
    if isinstance(e, ast.Col):
        return e.name
    if isinstance(e, ast.Func):
        inner = ",".join(_expr_name(a) for a in e.args)
        if e.distinct:
            inner = "DISTINCT " + inner
        return f"{e.name}({inner})"
    if isinstance(e, ast.Star):
        return "*"
    if isinstance(e, ast.Lit):
        return str(e.value)
    if isinstance(e, ast.BinOp):
        return f"{_expr_name(e.left)} {e.op} {_expr_name(e.right)}"
    if isinstance(e, ast.UnaryOp):
        return f"{e.op}{_expr_name(e.operand)}"
    if isinstance(e, ast.Case):
        return "case"
    if isinstance(e, ast.ScalarSubquery):
        return "(subquery)"
    if isinstance(e, ast.SysVar):
        return "@@" + e.name
    if isinstance(e, ast.Cast):
        return f"CAST({_expr_name(e.expr)} AS {e.type.upper()})"
    return repr(e)


QueryExecutor = Executor
