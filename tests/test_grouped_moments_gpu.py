"""Grouped two-pass moments on the device against cpu_ref.grouped_moments
within bounds derived from each case's data, the launcher's limits, and SQL
parity on a GPU engine."""

import pytest
import torch

import _moments_cases as C
from greptimedb_amd import ops
from greptimedb_amd.ops import cpu_ref
from greptimedb_amd.query.executor import Executor

pytestmark = pytest.mark.gpu

CASES = C.op_cases()
_REF: dict = {}


def _ref(name):
    """cpu_ref planes of a case, computed once and shared."""
    if name not in _REF:
        planes = [p.numpy() for p in cpu_ref.grouped_moments(
            C.torch_sources(CASES[name], "cpu"), CASES[name]["fx"],
            CASES[name]["fy"], CASES[name]["n_cells"])]
        _REF[name] = dict(zip(C.PLANES, planes))
    return _REF[name]


def _check(name, **kw):
    got = C.run_op_case(ops, CASES[name], device="cuda:0", **kw)
    C.check_planes(got, _ref(name), C.oracle_of(name, CASES[name])["A"])


def test_geometry_matches_case_sizes():
    from greptimedb_amd import _hip_ops
    assert (_hip_ops.AGG_TILE, _hip_ops.LDS_CELLS) == (C.AGG_TILE, C.LDS_CELLS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_cpu_ref(name):
    _check(name)


@pytest.mark.parametrize("name", C.LDS_VARIANTS)
@pytest.mark.parametrize("lds_cells", [0, 5])
def test_lower_lds_span_gives_the_same_answer(name, lds_cells):
    _check(name, lds_cells=lds_cells)


def test_constant_column_is_exact():
    n, mx, _my, m2x, _m2y, cxy, cx, _cy = C.run_op_case(
        ops, CASES["constant"], device="cuda:0")
    assert cx[0, [0, 2]].all() and not cx[0, [1, 3]].any()
    assert (mx[0, [0, 2]] == 0.1).all() and (m2x[0, [0, 2]] == 0.0).all()
    assert (cxy[1, [0, 2]] == 0.0).all() and (cxy[1, [1, 3]] != 0.0).all()


def test_limits():
    dev = "cuda:0"
    src = [(torch.zeros(1, dtype=torch.int32, device=dev),
            torch.ones((1, 1), dtype=torch.float64, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))]
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0], [1], 4)          # fy past field_idx
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [1], [0], 4)
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0], [0], 262145)
    with pytest.raises(RuntimeError):
        ops.grouped_moments(src, [0, 0, 0], [0, 0, 0], 87382)
    with pytest.raises(RuntimeError):
        ops.grouped_moments([(src[0][0], src[0][1].float(), src[0][2])], [0], [0], 1)
    with pytest.raises(RuntimeError):
        ops.grouped_moments([(src[0][0], src[0][1].cpu(), src[0][2])], [0], [0], 1)
    n, mx, my, m2x, m2y, cxy, cx, cy = ops.grouped_moments(src, [0], [0], 1)
    assert n.is_cuda and n.dtype == torch.int64 and cx.dtype == torch.bool
    assert n.item() == 1 and mx.item() == 1.0 and my.item() == 1.0
    assert m2x.item() == 0.0 and m2y.item() == 0.0 and cxy.item() == 0.0
    assert cx.item() is True and cy.item() is True
    # sources without rows launch nothing and report empty cells
    none = [(src[0][0][:0], src[0][1][:, :0], src[0][2])]
    planes = ops.grouped_moments(none, [0], [0], 3)
    assert planes[0].is_cuda and int(planes[0].sum()) == 0
    assert bool(torch.isnan(planes[1]).all()) and not bool(planes[6].any())
    assert float(planes[3].abs().sum()) == 0.0


def _on_off(ex, sql):
    old = Executor._device_moments
    try:
        Executor._device_moments = True
        on = ex.execute(sql)
        Executor._device_moments = False
        off = ex.execute(sql)
    finally:
        Executor._device_moments = old
    return on, off


def test_sql_parity_on_gpu_engine(gpu_engine):
    ex = Executor(gpu_engine)
    rows = C.build_moments_table(ex, gpu_engine.flush_all)
    plan = ex.execute("EXPLAIN SELECT h, corr(a, b) FROM mt GROUP BY h").columns[0][0]
    assert plan == "Plan: grouped-moments (two-pass, M=1, cells=5)"
    for case in C.SQL_CASES:
        plan = ex.execute("EXPLAIN " + case["sql"]).columns[0][0]
        if "plan" in case:
            assert plan == case["plan"]
        assert plan.startswith(("Plan: grouped-moments", "Plan: grouped-quantile"))
        on, off = _on_off(ex, case["sql"])
        C.check_sql_same(on, off, rows, case)
        C.check_sql_numpy(on, rows, case)
        C.check_sql_numpy(off, rows, case)


def test_sql_on_last_non_null_table_on_gpu_engine(gpu_engine):
    ex = Executor(gpu_engine)
    rows = C.build_moments_table(ex, gpu_engine.flush_all, name="ml", lnn=True)
    case = dict(C.SQL_CASES[1])
    case["sql"] = case["sql"].replace(" mt ", " ml ")
    on, off = _on_off(ex, case["sql"])
    C.check_sql_same(on, off, rows, case)
    C.check_sql_numpy(on, rows, case)
