"""HIP kernels (csrc/kernels.hip) at the shapes and edges where kernels go
wrong, against the independent oracles of tests/_oracles.py — not against
ops.cpu_ref, which tests/test_ops_edges_cpu.py checks on the same cases
(tests/_edge_cases.py). Runs on an MI355X.

Kernel branches reached here and nowhere else in the suite: the wide-tile
fallback, a non-zero LDS table offset and the 1024/1025-cell boundary of
field_bucket_agg_lds_kernel; tiles of AGG_TILE ± 1 rows; strided, repeated
and empty field lists; empty input; buckets below the origin; both quantile
selection paths of prom_range_eval_kernel on the same data and its second
grid-stride step; the bounded-window deferral of series_last; every bit
width of rle_expand_indices_kernel; the 0/1/63/64-bit widths and all special
payloads of gorilla_decode_kernel.
"""

import numpy as np
import pytest
import torch

import _edge_cases as ec
import _oracles as orc
from greptimedb_amd.engine import gorilla
from greptimedb_amd.ops import kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.as_tensor(a).to(DEV)


# ------------------------------------------------------------ ts_bucket_agg
@pytest.mark.parametrize("name", [n for n in ec.AGG_CASES if n != "empty"])
def test_ts_bucket_agg(name):
    ec.check_agg(ec.run_agg(name, DEV), ec.agg_case(name)[2])


def test_ts_bucket_agg_empty_input():
    """n == 0 launches nothing and leaves the device usable."""
    got = ec.run_agg("empty", DEV)
    torch.cuda.synchronize()
    assert int((torch.arange(10, device=DEV) * 2).sum().item()) == 90
    ec.check_agg(got, ec.agg_case("empty")[2])
    assert not got[0].any() and not got[4].any() and np.isnan(got[2]).all()


def test_ts_bucket_agg_empty_source_between_sources():
    """An empty source in the middle of an accumulation changes nothing."""
    chunks, args, exp = ec.agg_case("acc3")
    empty = {k: (v[:, :0] if k == "fields" else v[:0] if k in ("ts", "series")
                 else v) for k, v in chunks[0].items()}
    acc = None
    for c in (chunks[0], empty, chunks[1], chunks[2]):
        acc = kernels.ts_bucket_agg_acc(
            _dev(c["ts"]), _dev(np.ascontiguousarray(c["series"])),
            _dev(np.ascontiguousarray(c["fields"])), _dev(c["field_idx"]),
            _dev(c["lut"]), *args, acc=acc)
    torch.cuda.synchronize()
    ec.check_agg([o.cpu().numpy() for o in kernels.ts_bucket_agg_finish(acc)],
                 exp)


def test_agg_extremes_exact_minmax():
    got = ec.run_agg("extremes", DEV)
    assert got[2][0, :, 0].tolist() == [-1e308, -5e-324, 0.0]
    assert got[3][0, :, 0].tolist() == [1e308, 5e-324, 0.0]


# ---------------------------------------------------------- prom_range_eval
@pytest.mark.parametrize("name,mode,param,with_nan",
                         ec.prom_modes(), ids=[m[0] for m in ec.prom_modes()])
def test_prom_range_eval(name, mode, param, with_nan):
    d = ec.prom_data()
    exp, tol = ec.prom_expected(mode, param, with_nan)
    got = ec.run_prom(d, d["vals_nan" if with_nan else "vals"], ec.PROM_GRID,
                      param, mode, DEV)
    ec.check_prom(got, exp, tol, mode)


def test_prom_grid_stride_count_last():
    data, count, last = ec.prom_wide()
    for mode, exp in ((orc.COUNT, count), (orc.LAST, last)):
        got = ec.run_prom(data, data["vals"], ec.PROM_WIDE_GRID, 0.0, mode, DEV)
        np.testing.assert_array_equal(got, exp)


# -------------------------------------------------------------- series_last
@pytest.mark.parametrize("window", [ec.UNBOUNDED, ec.BOUNDED],
                         ids=["unbounded", "bounded"])
def test_series_last(window):
    exp = ec.series_last_expected(window)
    got = ec.run_series_last(window, DEV)
    for e, g, name in zip(exp, got, ("ts", "src", "row")):
        np.testing.assert_array_equal(g, e, err_msg=name)


# --------------------------------------------------------------- RLE expand
def _rle_gpu(runs, blob, bw, n):
    from greptimedb_amd import _hip_ops
    padded = np.frombuffer(blob + b"\x00" * 16, dtype=np.uint8).copy()
    return _hip_ops.rle_expand_indices(_dev(runs), _dev(padded), bw,
                                       n).cpu().numpy()


@pytest.mark.parametrize("bw", range(1, 33))
def test_rle_expand(bw):
    runs, blob, n, values = ec.rle_case(bw)
    got = _rle_gpu(runs, blob, bw, n)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, orc.rle_expand(runs, blob, bw, n))
    np.testing.assert_array_equal(got, values)


def test_rle_expand_one_long_run():
    runs, blob, n, values = ec.rle_case_big()
    assert n == ec.GRID_SPAN + 1
    np.testing.assert_array_equal(_rle_gpu(runs, blob, 13, n), values)


# ------------------------------------------------------------------ gorilla
@pytest.mark.parametrize("ts_kind,val_kind,block,pack_ts", ec.GORILLA_CASES)
def test_gorilla_decode(ts_kind, val_kind, block, pack_ts):
    ts, vals, packed = ec.gorilla_case(ts_kind, val_kind, block, pack_ts)
    got_ts, got_vals = gorilla.decode(*packed, DEV)
    assert got_ts.is_cuda and got_vals.is_cuda
    ec.check_gorilla(ts, vals, packed, block, pack_ts,
                     got_ts.cpu().numpy(), got_vals.cpu().numpy())


# ------------------------------------------------- filter / dedup / scatter
@pytest.mark.parametrize("n", ec.SMALL_SIZES)
@pytest.mark.parametrize("use_lut", [True, False])
def test_filter_series_time(n, use_lut):
    ts, series, lut = ec.rows_case(n)
    got = kernels.filter_series_time(
        _dev(ts), _dev(series), _dev(lut) if use_lut else None, -20, 30)
    assert got.is_cuda
    np.testing.assert_array_equal(
        got.cpu().numpy(),
        orc.filter_series_time(ts, series, lut if use_lut else None, -20, 30))


@pytest.mark.parametrize("n", ec.SMALL_SIZES)
def test_dedup_mark_last(n):
    ts, series, _ = ec.rows_case(n)
    got = kernels.dedup_mark_last(_dev(series), _dev(ts))
    assert got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(),
                                  orc.dedup_mark_last(series, ts))


@pytest.mark.parametrize("n", (0, 1, 257))
@pytest.mark.parametrize("R", (1, 3))
def test_scatter_append(n, R):
    got, exp = ec.run_scatter(n, R, DEV)
    for g_list, e_list in zip(got, exp):
        for g, e in zip(g_list, e_list):
            np.testing.assert_array_equal(g, e)
