"""merge_mode = 'last_non_null' on the CPU: the op's reference against a loop
oracle, the SQL surface in every storage state, the table option's life
cycle, and the compaction picker's sequence-closure rule."""

import json
import os

import numpy as np
import pytest
import torch

import _lnn_cases as L
from greptimedb_amd.engine import compaction
from greptimedb_amd.engine.compaction import Compactor, close_over_sequences
from greptimedb_amd.engine.engine import EngineConfig, MitoEngine
from greptimedb_amd.ops import cpu_ref, merge_last_non_null
from greptimedb_amd.query.executor import Executor
from greptimedb_amd.utils.errors import InvalidArguments


# ------------------------------------------------------------------- op

@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_cpu_ref_matches_loop_oracle(name):
    se, ts, f, kidx, merged = L.cases()[name]
    args = (torch.as_tensor(se.copy()), torch.as_tensor(ts.copy()),
            torch.as_tensor(f.copy()))
    got_k, got_m = cpu_ref.merge_last_non_null(*args)
    L.check(got_k.numpy(), got_m.numpy(), kidx, merged)
    # the dispatch layer takes CPU tensors to the same function
    got_k, got_m = merge_last_non_null(*args)
    L.check(got_k.numpy(), got_m.numpy(), kidx, merged)
    np.testing.assert_array_equal(
        got_k.numpy(),
        cpu_ref.dedup_mark_last(args[0], args[1]).nonzero(
            as_tuple=True)[0].numpy())


# ------------------------------------------------------------------ SQL

def _flush_regions(eng):
    """Flush every region without the post-flush compaction check that
    MitoEngine.flush_all runs, so a test decides when files are merged."""
    for st in eng.tables.values():
        for r in st.regions:
            r.flush()


def _compact_all(eng, table):
    return sum(Compactor().compact_region(r)
               for r in eng.table(table).regions)


def _run_steps(ex, after_insert):
    ex.execute(L.CREATE_LNN)
    ex.execute(L.CREATE_LR)
    for ins, exp_lnn, exp_lr in L.STEPS:
        ex.execute("INSERT INTO lnn VALUES " + ins)
        ex.execute("INSERT INTO lr VALUES " + ins)
        after_insert()
        assert L.select_rows(ex, "lnn") == exp_lnn
        assert L.select_rows(ex, "lr") == exp_lr


def test_sql_memtable_only(tmp_engine):
    _run_steps(Executor(tmp_engine), lambda: None)


def test_sql_after_flush_and_compaction(tmp_engine):
    eng = tmp_engine
    ex = Executor(eng)
    _run_steps(ex, lambda: _flush_regions(eng))   # every step reads SSTs only
    final_lnn, final_lr = L.STEPS[-1][1], L.STEPS[-1][2]
    files_before = sum(len(r.manifest.files) for r in eng.table("lnn").regions)
    assert files_before >= 4                # host1's region: one per insert
    assert _compact_all(eng, "lnn") >= 1
    assert _compact_all(eng, "lr") >= 1
    assert sum(len(r.manifest.files)
               for r in eng.table("lnn").regions) < files_before
    assert L.select_rows(ex, "lnn") == final_lnn
    assert L.select_rows(ex, "lr") == final_lr
    # a partial write on top of the compacted file still merges
    ex.execute("INSERT INTO lnn VALUES ('host2', 1, NULL, 7)")
    assert L.select_rows(ex, "lnn") == [("host1", 0, 20.0, 10.0),
                                        ("host2", 1, 11.0, 7.0)]


def test_sql_flush_between_steps(tmp_engine):
    """SST + live memtable: flush after the second insert only."""
    eng = tmp_engine
    ex = Executor(eng)
    n = [0]

    def after():
        n[0] += 1
        if n[0] == 2:
            eng.flush_all()
    _run_steps(ex, after)
    # only the merged row satisfies both predicates: cpu = 20 arrived in one
    # write and memory = 10 in another
    assert L.select_rows(ex, "lnn", "WHERE cpu > 15 AND memory > 5") == \
        [("host1", 0, 20.0, 10.0)]
    assert L.select_rows(ex, "lr", "WHERE cpu > 15 AND memory > 5") == []
    assert L.select_rows(ex, "lnn", "WHERE cpu > 15") == \
        [("host1", 0, 20.0, 10.0)]
    r = ex.execute("SELECT host, count(cpu), avg(cpu), count(memory), "
                   "avg(memory), count(*) FROM lnn GROUP BY host "
                   "ORDER BY host")
    assert [list(c) for c in r.columns] == [
        ["host1", "host2"], [1, 1], [20.0, 11.0], [1, 1], [10.0, 1.0], [1, 1]]
    r = ex.execute("SELECT host, count(cpu), count(memory), count(*) FROM lr "
                   "GROUP BY host ORDER BY host")
    assert [list(c) for c in r.columns] == [
        ["host1", "host2"], [0, 1], [0, 0], [1, 1]]


def _names(ex, table):
    r = ex.execute(f"SELECT ts, code, name, status FROM {table} ORDER BY ts")
    return [(c, n, None if s is None or np.isnan(s) else float(s))
            for c, n, s in zip(r.columns[1], r.columns[2], r.columns[3])]


def test_sql_delete_then_reinsert_fewer_columns(tmp_engine):
    eng = tmp_engine
    ex = Executor(eng)
    ex.execute("CREATE TABLE db (ts TIMESTAMP TIME INDEX, code STRING, "
               "name STRING, status TINYINT, PRIMARY KEY (code)) "
               "WITH (merge_mode = 'last_non_null')")
    assert eng.table("db").regions[0].text_cols == {}
    files = ["1.png", "2.png", "3.png"]
    for i, nm in enumerate(files):
        ex.execute("INSERT INTO db (ts, code, name, status) VALUES "
                   f"('2024-11-26 10:0{i}:00', 'achn', '{nm}', {i // 2})")
    assert _names(ex, "db") == [("achn", "1.png", 0.0), ("achn", "2.png", 0.0),
                                ("achn", "3.png", 1.0)]
    assert ex.execute("DELETE FROM db").columns[0][0] == 3
    assert _names(ex, "db") == []
    for i, nm in enumerate(files):
        ex.execute("INSERT INTO db (ts, code, name) VALUES "
                   f"('2024-11-26 10:0{i}:00', 'achn', '{nm}')")
    exp = [("achn", nm, None) for nm in files]
    assert _names(ex, "db") == exp          # the deleted status stays gone
    eng.flush_all()
    assert _names(ex, "db") == exp


def test_sql_string_field_merges(tmp_engine):
    """A plain string field keeps its newest non-NULL value like a number,
    in the memtable, across SSTs and through compaction."""
    eng = tmp_engine
    ex = Executor(eng)
    ex.execute("CREATE TABLE sm (ts TIMESTAMP TIME INDEX, code STRING, "
               "name STRING, status DOUBLE, PRIMARY KEY (code)) "
               "WITH ('merge_mode'='last_non_null')")
    ex.execute("INSERT INTO sm (ts, code, name) VALUES (1000, 'a', 'first')")
    ex.execute("INSERT INTO sm (ts, code, status) VALUES (1000, 'a', 4)")
    ex.execute("INSERT INTO sm (ts, code, name) VALUES (2000, 'a', 'other')")
    exp = [("a", "first", 4.0), ("a", "other", None)]
    assert _names(ex, "sm") == exp
    eng.flush_all()
    assert _names(ex, "sm") == exp
    ex.execute("INSERT INTO sm (ts, code, status) VALUES (2000, 'a', 5)")
    exp2 = [("a", "first", 4.0), ("a", "other", 5.0)]
    assert _names(ex, "sm") == exp2         # SST + memtable
    _flush_regions(eng)
    ex.execute("INSERT INTO sm (ts, code, name) VALUES (1000, 'a', 'second')")
    _flush_regions(eng)
    ex.execute("INSERT INTO sm (ts, code, status) VALUES (3000, 'a', 6)")
    _flush_regions(eng)
    exp3 = [("a", "second", 4.0), ("a", "other", 5.0), ("a", None, 6.0)]
    assert _names(ex, "sm") == exp3         # four SSTs
    assert _compact_all(eng, "sm") == 1
    assert _names(ex, "sm") == exp3


# --------------------------------------------------------------- option

COLS = "(h STRING, ts TIMESTAMP TIME INDEX, v DOUBLE, PRIMARY KEY (h))"


def test_invalid_merge_mode_value(tmp_engine):
    ex = Executor(tmp_engine)
    with pytest.raises(InvalidArguments, match="first_row"):
        ex.execute(f"CREATE TABLE bad {COLS} WITH ('merge_mode'='first_row')")
    assert "bad" not in tmp_engine.tables


def test_last_non_null_rejects_append_mode(tmp_engine):
    ex = Executor(tmp_engine)
    with pytest.raises(InvalidArguments, match="append_mode"):
        ex.execute(f"CREATE TABLE bad {COLS} WITH "
                   "('merge_mode'='last_non_null', 'append_mode'='true')")
    assert "bad" not in tmp_engine.tables
    # last_row with append_mode stays legal
    ex.execute(f"CREATE TABLE ok {COLS} WITH "
               "('merge_mode'='last_row', 'append_mode'='true')")
    assert tmp_engine.table("ok").append_mode


def test_last_non_null_rejects_fulltext(tmp_engine):
    ex = Executor(tmp_engine)
    with pytest.raises(InvalidArguments, match="FULLTEXT"):
        ex.execute("CREATE TABLE bad (h STRING, ts TIMESTAMP TIME INDEX, "
                   "msg STRING FULLTEXT INDEX, PRIMARY KEY (h)) "
                   "WITH ('merge_mode'='last_non_null')")
    assert "bad" not in tmp_engine.tables


def test_show_create_table(tmp_engine):
    ex = Executor(tmp_engine)
    ex.execute(L.CREATE_LNN)
    ex.execute(L.CREATE_LR)
    ex.execute(f"CREATE TABLE plain {COLS}")
    ddl = {t: ex.execute(f"SHOW CREATE TABLE {t}").columns[1][0]
           for t in ("lnn", "lr", "plain")}
    assert ddl["lnn"].count("merge_mode = 'last_non_null'") == 1
    assert "merge_mode" not in ddl["lr"]
    assert "merge_mode" not in ddl["plain"]
    st = tmp_engine.table("lnn")
    assert st.merge_mode == "last_non_null"
    assert all(r.merge_mode == "last_non_null" for r in st.regions)
    assert tmp_engine.table("lr").merge_mode == "last_row"
    assert tmp_engine.table("plain").merge_mode == "last_row"
    assert all(r.merge_mode == "last_row"
               for r in tmp_engine.table("plain").regions)


def test_reopen_keeps_mode_and_old_catalog_loads_as_last_row(tmp_path):
    cfg = EngineConfig(data_dir=str(tmp_path / "data"), device="cpu",
                       background_flush=False)
    eng = MitoEngine(cfg)
    ex = Executor(eng)
    n = [0]

    def after():
        n[0] += 1
        if n[0] == 2:
            eng.flush_all()
    _run_steps(ex, after)                   # SST on disk, the rest in the WAL
    eng.close()

    cat_path = os.path.join(cfg.data_dir, "catalog.json")
    with open(cat_path) as f:
        cat = json.load(f)
    assert {td["schema"]["name"]: td["merge_mode"] for td in cat["tables"]} \
        == {"lnn": "last_non_null", "lr": "last_row"}

    eng = MitoEngine(cfg)
    try:
        st = eng.table("lnn")
        assert st.merge_mode == "last_non_null"
        assert all(r.merge_mode == "last_non_null" for r in st.regions)
        assert eng.table("lr").merge_mode == "last_row"
        ex = Executor(eng)
        assert L.select_rows(ex, "lnn") == L.STEPS[-1][1]
        assert L.select_rows(ex, "lr") == L.STEPS[-1][2]
    finally:
        eng.close()

    # a catalog written before the option existed has no key at all
    for td in cat["tables"]:
        del td["merge_mode"]
    with open(cat_path, "w") as f:
        json.dump(cat, f)
    eng = MitoEngine(cfg)
    try:
        for t in ("lnn", "lr"):
            assert eng.table(t).merge_mode == "last_row"
            assert all(r.merge_mode == "last_row"
                       for r in eng.table(t).regions)
        # and reads as LastRow: the SST holds the rows merged at flush time
        # (host1 0/10, host2 11/1); host1's newer all-NULL write in the WAL
        # now wins as a whole row
        assert L.select_rows(Executor(eng), "lnn") == [
            ("host1", 0, None, None), ("host2", 1, 11.0, 1.0)]
    finally:
        eng.close()


def test_create_table_api_takes_merge_mode(tmp_engine):
    from greptimedb_amd.models.schema import (ColumnSchema, DataType,
                                              SemanticType, TableSchema)
    cols = [ColumnSchema("h", DataType.STRING, SemanticType.TAG, 0),
            ColumnSchema("ts", DataType.TIMESTAMP_MS, SemanticType.TIMESTAMP, 1),
            ColumnSchema("v", DataType.FLOAT64, SemanticType.FIELD, 2)]
    st = tmp_engine.create_table(
        TableSchema(name="api", columns=cols, primary_key=["h"]),
        n_regions=1, merge_mode="last_non_null")
    assert st.merge_mode == "last_non_null"
    assert st.regions[0].merge_mode == "last_non_null"
    with pytest.raises(InvalidArguments):
        tmp_engine.create_table(
            TableSchema(name="api2", columns=cols, primary_key=["h"]),
            merge_mode="newest")


# ------------------------------------------------- compaction closure rule

def _meta(lo, hi, seq):
    return {"min_ts": lo, "max_ts": hi, "seq_max": seq, "level": 0}


def test_close_over_sequences_unit():
    files = {"f1": _meta(0, 10, 1), "f2": _meta(5, 15, 2),
             "f3": _meta(0, 10, 3),
             "far": _meta(100, 110, 2),     # interleaved but disjoint in time
             "new": _meta(0, 10, 9)}        # overlapping but newer than all
    assert close_over_sequences(files, ["f1", "f3"]) == ["f1", "f3", "f2"]
    assert close_over_sequences(files, ["f1", "f2"]) == ["f1", "f2"]
    # transitive: pulling f2 in widens the time range to reach `mid`
    files2 = {"a": _meta(0, 10, 1), "b": _meta(10, 30, 4), "c": _meta(0, 5, 6),
              "mid": _meta(25, 40, 3)}
    assert sorted(close_over_sequences(files2, ["a", "c"])) == \
        ["a", "b", "c", "mid"]
    many = {f"g{i}": _meta(0, 10, i) for i in range(compaction.MAX_INPUTS + 2)}
    assert close_over_sequences(
        many, ["g0", f"g{compaction.MAX_INPUTS + 1}"]) is None


class _ForcedPicker(Compactor):
    """Proposes one fixed group, as a time-window picker with a file cap
    could; pick() still has to close it for a last_non_null region."""

    def __init__(self, group):
        super().__init__()
        self.group = group

    def _window_groups(self, region):
        return [list(self.group)]


def _three_files(ex, eng, table):
    """Files 1, 2, 3 holding cpu = 1, 2, NULL for one key; returns the
    key's region and its file ids in sequence order."""
    for cpu, mem in (("1", "NULL"), ("2", "NULL"), ("NULL", "5")):
        ex.execute(f"INSERT INTO {table} VALUES ('host1', 0, {cpu}, {mem})")
        eng.flush_all()
    (region,) = [r for r in eng.table(table).regions if r.manifest.files]
    fids = sorted(region.manifest.files,
                  key=lambda f: region.manifest.files[f]["seq_max"])
    assert len(fids) == 3
    return region, fids


def test_compaction_pulls_in_the_interleaved_file(tmp_engine):
    eng = tmp_engine
    ex = Executor(eng)
    ex.execute(L.CREATE_LNN)
    ex.execute(L.CREATE_LR)
    region, (f1, f2, f3) = _three_files(ex, eng, "lnn")
    picker = _ForcedPicker([f1, f3])
    assert [sorted(g) for g in picker.pick(region)] == [sorted([f1, f2, f3])]
    assert picker.compact_region(region) == 1
    assert len(region.manifest.files) == 1
    assert L.select_rows(ex, "lnn") == [("host1", 0, 2.0, 5.0)]
    # LastRow picking is unchanged: the proposed pair is merged as it is
    region_lr, (g1, g2, g3) = _three_files(ex, eng, "lr")
    picker = _ForcedPicker([g1, g3])
    assert picker.pick(region_lr) == [[g1, g3]]
    assert picker.compact_region(region_lr) == 1
    assert set(region_lr.manifest.files) - {g2} != set()
    assert g2 in region_lr.manifest.files
    assert L.select_rows(ex, "lr") == [("host1", 0, None, 5.0)]
