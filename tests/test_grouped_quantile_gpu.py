"""Grouped radix-histogram selection on the device against the per-cell
numpy oracle (bitwise), its limits, and SQL parity on a GPU engine."""

import pytest
import torch

import _quantile_cases as C
from greptimedb_amd import ops
from greptimedb_amd.query.executor import Executor

pytestmark = pytest.mark.gpu

CASES = C.op_cases()


def test_launch_config_matches_case_sizes():
    from greptimedb_amd import _hip_ops
    assert tuple(_hip_ops.quantile_launch_config()) == C.LAUNCH_CFG


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_numpy_oracle(name):
    C.check_op_case(ops, CASES[name], device="cuda:0")


@pytest.mark.parametrize("name", ["sorted_lds", "multi_source", "span_cap"])
@pytest.mark.parametrize("lds_cells", [0, 5])
def test_lower_lds_span_gives_the_same_answer(name, lds_cells):
    C.check_op_case(ops, CASES[name], device="cuda:0", lds_cells=lds_cells)


def test_bucket_cells_matches_cpu_ref():
    import numpy as np
    from greptimedb_amd.ops import cpu_ref
    rng = np.random.default_rng(2)
    n = 5000
    ts = torch.from_numpy(rng.integers(-50, 1000, n))
    series = torch.from_numpy(rng.integers(-1, 8, n).astype(np.int32))
    lut = torch.tensor([0, -1, 1, 2, -1, 0], dtype=torch.int32)
    want = cpu_ref.bucket_cells(ts, series, lut, 10, 900, 0, 100, 9)
    got = ops.bucket_cells(ts.cuda(), series.cuda(), lut.cuda(), 10, 900, 0, 100, 9)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    empty = ops.bucket_cells(ts[:0].cuda(), series[:0].cuda(), lut.cuda(),
                             10, 900, 0, 100, 9)
    assert empty.numel() == 0


def test_limits():
    dev = "cuda:0"
    src = [(torch.zeros(1, dtype=torch.int32, device=dev),
            torch.ones((1, 1), dtype=torch.float64, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))]
    with pytest.raises(RuntimeError):
        ops.grouped_quantile(src, [0], [0.5], 262145)
    with pytest.raises(RuntimeError):
        ops.grouped_quantile(src, [0, 0, 0], [0.5, 0.6, 0.7], 87382)
    with pytest.raises(RuntimeError):
        ops.grouped_quantile(src, [1], [0.5], 4)       # field_of_sel past field_idx
    lo, hi, cnt = ops.grouped_quantile(src, [0], [0.5], 1)
    assert lo.is_cuda and lo.item() == 1.0 and hi.item() == 1.0 and cnt.item() == 1
    # sources without rows launch nothing and report empty cells
    none = [(src[0][0][:0], src[0][1][:, :0], src[0][2])]
    lo, hi, cnt = ops.grouped_quantile(none, [0], [0.5], 3)
    assert lo.is_cuda and bool(torch.isnan(lo).all()) and int(cnt.sum()) == 0


def test_on_pass_is_called_between_passes():
    dev = "cuda:0"
    src = [(torch.zeros(4, dtype=torch.int32, device=dev),
            torch.arange(4, dtype=torch.float64, device=dev).reshape(1, 4),
            torch.zeros(1, dtype=torch.int32, device=dev))]
    calls = []
    ops.grouped_quantile(src, [0], [0.5], 1, on_pass=lambda: calls.append(1))
    assert len(calls) == 8


def test_sql_parity_on_gpu_engine(gpu_engine):
    ex = Executor(gpu_engine)
    C.build_parity_table(ex, gpu_engine.flush_all)
    for sql in C.PARITY_QUERIES:
        plan = ex.execute("EXPLAIN " + sql).columns[0][0]
        assert plan.startswith("Plan: grouped-quantile"), plan
        old = Executor._device_quantile
        try:
            Executor._device_quantile = True
            on = ex.execute(sql)
            Executor._device_quantile = False
            off = ex.execute(sql)
        finally:
            Executor._device_quantile = old
        C.assert_same_result(on, off, sql)
