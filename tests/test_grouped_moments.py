"""Grouped second moments (var / stddev / covar / corr): the CPU reference op
against a per-cell numpy oracle, SQL parity between the device plan and the
host path on a CPU-device engine, values against numpy, and routing."""

import numpy as np
import pytest
import torch

import _moments_cases as C
from greptimedb_amd import ops
from greptimedb_amd.ops import cpu_ref
from greptimedb_amd.query.executor import Executor

CASES = C.op_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_ref_matches_numpy_oracle(name):
    ref = C.oracle_of(name, CASES[name])
    C.check_planes(C.run_op_case(ops, CASES[name]), ref, ref["A"])


def test_constant_column_is_exact():
    case = CASES["constant"]
    n, mx, _my, m2x, _m2y, cxy, cx, cy = C.run_op_case(ops, case)
    assert cx[0, [0, 2]].all() and not cx[0, [1, 3]].any() and not cy[1].any()
    assert (mx[0, [0, 2]] == 0.1).all() and (m2x[0, [0, 2]] == 0.0).all()
    planes = [p[1] for p in (n, mx, _my, m2x, _m2y, cxy, cx, cy)]   # (0.1, y)
    val, null = cpu_ref.moments_finish("corr", planes)
    assert list(null) == [True, False, True, False]
    val, null = cpu_ref.moments_finish("var_samp", [p[0] for p in
                                                    (n, mx, _my, m2x, _m2y, cxy, cx, cy)])
    assert not null.any() and val[0] == 0.0 and val[2] == 0.0


def test_offset_rejects_raw_sum_of_squares():
    """sum(x^2) - n*mean^2 at |x| ~ 1e9 is off by far more than the bound
    allows, so a single-pass formulation cannot pass the `offset` case."""
    case = CASES["offset"]
    ref = C.oracle_of("offset", case)
    c, x, _y = C._pairs(case, 1)
    naive = np.array([np.sum(x[c == i] ** 2) - np.sum(x[c == i]) ** 2 / 1000
                      for i in range(8)])
    b = C.bounds(ref["n"][1], ref["A"][1], ref["m2x"][1], ref["m2y"][1])
    assert (np.abs(naive - ref["m2x"][1]) > 100 * b["m2x"]).all()


def test_moments_finish_null_rules():
    def planes(n, m2x=2.0, m2y=8.0, cxy=-5.0, cx=False, cy=False):
        return [np.array([v]) for v in (n, 0.0, 0.0, m2x, m2y, cxy, cx, cy)]
    want_null = {0: set(C.KINDS),
                 1: {"var_samp", "stddev_samp", "covar_samp", "covar", "corr"},
                 2: set()}
    for n, nulls in want_null.items():
        for kind in C.KINDS:
            val, null = cpu_ref.moments_finish(kind, planes(n))
            assert bool(null[0]) == (kind in nulls), (n, kind)
            assert np.isnan(val[0]) == (kind in nulls)
    p4 = planes(4)
    assert cpu_ref.moments_finish("var_pop", p4)[0][0] == 0.5
    assert cpu_ref.moments_finish("var_samp", p4)[0][0] == 2.0 / 3
    assert cpu_ref.moments_finish("stddev_pop", p4)[0][0] == np.sqrt(0.5)
    assert cpu_ref.moments_finish("covar_pop", p4)[0][0] == -1.25
    assert cpu_ref.moments_finish("covar", p4)[0][0] == -5.0 / 3
    assert cpu_ref.moments_finish("corr", planes(4, cxy=-4.0))[0][0] == -1.0
    assert cpu_ref.moments_finish("corr", planes(4, cxy=4.5))[0][0] == 1.0   # clamp
    for flag in ("cx", "cy"):
        assert cpu_ref.moments_finish("corr", planes(4, **{flag: True}))[1][0]
        assert not cpu_ref.moments_finish("covar", planes(4, **{flag: True}))[1][0]
    with pytest.raises(ValueError):
        cpu_ref.moments_finish("stddev", p4)


def test_limits():
    src = [(torch.zeros(1, dtype=torch.int32), torch.ones((1, 1), dtype=torch.float64),
            torch.zeros(1, dtype=torch.int32))]
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0], [1], 4)               # fy past field_idx
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0], [0], 262145)
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0, 0, 0], [0, 0, 0], 87382)
    n, mx, my, m2x, m2y, cxy, cx, cy = ops.grouped_moments(src, [0], [0], 1)
    assert n.item() == 1 and mx.item() == 1.0 and m2x.item() == 0.0
    assert cx.item() is True and cy.item() is True
    planes = ops.grouped_moments([], [0, 0], [0, 0], 3)
    assert planes[0].shape == (2, 3) and int(planes[0].sum()) == 0
    assert bool(torch.isnan(planes[1]).all()) and not bool(planes[6].any())


# ---------------------------------------------------------------- SQL

@pytest.fixture
def mex(tmp_engine):
    ex = Executor(tmp_engine)
    rows = C.build_moments_table(ex, tmp_engine.flush_all)
    return ex, rows


def _run(ex, sql, device_plan):
    old = Executor._device_moments
    Executor._device_moments = device_plan
    try:
        return ex.execute(sql)
    finally:
        Executor._device_moments = old


def test_table_shape(mex):
    ex, rows = mex
    assert Executor._device_moments is True
    assert len(ex.execute("SELECT * FROM mt")) == len(rows) == 200
    st = ex.engine.table("mt")
    assert any(len(r.scan_sources()) >= 2 for r in st.regions)


@pytest.mark.parametrize("case", C.SQL_CASES, ids=lambda c: c["sql"][7:60])
def test_sql_device_plan_vs_host_path_vs_numpy(mex, case):
    ex, rows = mex
    sql = case["sql"]
    plan = ex.execute("EXPLAIN " + sql).columns[0][0]
    if "plan" in case:
        assert plan == case["plan"]
    elif "approx_percentile" in sql:
        assert plan.startswith("Plan: grouped-quantile (radix select, Q=") and \
            ", moments M=" in plan
    else:
        assert plan.startswith("Plan: grouped-moments (two-pass, M="), plan
    on, off = _run(ex, sql, True), _run(ex, sql, False)
    C.check_sql_same(on, off, rows, case)
    C.check_sql_numpy(off, rows, case)
    C.check_sql_numpy(on, rows, case)


def test_sql_on_last_non_null_table(tmp_engine):
    ex = Executor(tmp_engine)
    rows = C.build_moments_table(ex, tmp_engine.flush_all, name="ml", lnn=True)
    case = dict(C.SQL_CASES[1])
    case["sql"] = case["sql"].replace(" mt ", " ml ")
    assert ex.execute("EXPLAIN " + case["sql"]).columns[0][0].startswith(
        "Plan: grouped-moments")
    on, off = _run(ex, case["sql"], True), _run(ex, case["sql"], False)
    C.check_sql_same(on, off, rows, case)
    C.check_sql_numpy(off, rows, case)


def _spy(monkeypatch):
    taken = []
    dev, host = Executor._exec_device_quantile, Executor._exec_sketch_select

    def spy_dev(self, dq):
        taken.append("device")
        return dev(self, dq)

    def spy_host(self, sel):
        taken.append("host")
        return host(self, sel)
    monkeypatch.setattr(Executor, "_exec_device_quantile", spy_dev)
    monkeypatch.setattr(Executor, "_exec_sketch_select", spy_host)
    return taken


def test_routing(mex, monkeypatch):
    ex, _rows = mex
    taken = _spy(monkeypatch)
    sql = "SELECT h, corr(a, b) FROM mt GROUP BY h"
    assert "grouped-moments" in ex.execute("EXPLAIN " + sql).columns[0][0]
    ex.execute(sql)
    assert taken == ["device"]
    del taken[:]
    for other in ["SELECT h, corr(a, b), stddev(a) FROM mt GROUP BY h",
                  "SELECT h, corr(a, a + b) FROM mt GROUP BY h",
                  "SELECT upper(h), var_pop(a) FROM mt GROUP BY h"]:
        assert "grouped-" not in ex.execute("EXPLAIN " + other).columns[0][0]
        ex.execute(other)
    assert taken == ["host"] * 3
    del taken[:]
    monkeypatch.setattr(Executor, "_device_moments", False)
    assert "grouped-" not in ex.execute("EXPLAIN " + sql).columns[0][0]
    mixed = "SELECT h, corr(a, b), median(a) FROM mt GROUP BY h"
    assert "grouped-" not in ex.execute("EXPLAIN " + mixed).columns[0][0]
    assert "grouped-quantile" in ex.execute(
        "EXPLAIN SELECT h, median(a) FROM mt GROUP BY h").columns[0][0]
    ex.execute(sql)
    ex.execute(mixed)
    assert taken == ["host", "host"]


def _by_host(rows):
    out = {}
    for r in rows:
        out.setdefault(r["h"], []).append(r)
    return out


def test_distinct_and_join_take_the_host_path(mex, monkeypatch):
    ex, rows = mex
    taken = _spy(monkeypatch)
    case = dict(sql="SELECT DISTINCT h, corr(a, b), var_samp(a) FROM mt GROUP BY h",
                key=C._h, cols={1: ("corr", "a", "b"), 2: ("var_samp", "a", "a")})
    assert "grouped-" not in ex.execute("EXPLAIN " + case["sql"]).columns[0][0]
    C.check_sql_numpy(ex.execute(case["sql"]), rows, case)
    assert taken == ["host"]
    # every row of x meets every row of y with the same h and dc
    r = ex.execute("SELECT x.h, covar_pop(x.a, y.b), stddev_samp(y.a) FROM mt x "
                   "JOIN mt y ON x.h = y.h AND x.dc = y.dc GROUP BY x.h")
    assert taken == ["host"] and len(r) == 5
    for (h, cov, sd), (h2, rs) in zip(r.rows(), sorted(_by_host(rows).items())):
        assert h == h2
        xs, ys, ya = [], [], []
        for p in rs:
            for q in rs:
                if p["dc"] == q["dc"]:
                    xs.append(p["a"]), ys.append(q["b"]), ya.append(q["a"])
        xs, ys, ya = np.array(xs), np.array(ys), np.array(ya)
        n = len(xs)
        wc, wsd = float(np.cov(xs, ys, ddof=0)[0, 1]), float(np.std(ya, ddof=1))
        A = max(np.abs(xs).max(), np.abs(ys).max())
        tol = C.value_bound("covar_pop", n, A, np.var(xs) * n, np.var(ys) * n, wc)
        assert abs(cov - wc) <= tol
        tol = C.value_bound("stddev_samp", n, np.abs(ya).max(), np.var(ya) * n,
                            np.var(ya) * n, wsd)
        assert abs(sd - wsd) <= tol


def test_stddev_and_var_keep_their_meaning(mex):
    ex, rows = mex
    r = ex.execute("SELECT stddev(a), var(a) FROM mt")
    a = np.array([row["a"] for row in rows])
    assert np.isclose(r.columns[0][0], np.std(a), rtol=1e-12, atol=0)
    assert np.isclose(r.columns[1][0], np.var(a), rtol=1e-12, atol=0)
    r = ex.execute("SELECT h, stddev(a) FROM mt GROUP BY h")
    for (h, sd), (h2, rs) in zip(r.rows(), sorted(_by_host(rows).items())):
        assert h == h2
        assert np.isclose(sd, np.std([p["a"] for p in rs]), rtol=1e-12, atol=0)
