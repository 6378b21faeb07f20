"""The CPU reference ops (ops.cpu_ref), the cold-tier codec's CPU side
(gorilla.pack / decode_ref) and pagedec._expand_cpu against the independent
oracles in tests/_oracles.py, on the cases of tests/_edge_cases.py — the same
ones tests/test_ops_gpu_edges.py runs through the HIP kernels. No GPU needed.
"""

import numpy as np
import pytest
import torch

import _edge_cases as ec
import _oracles as orc
from greptimedb_amd.engine import gorilla, pagedec
from greptimedb_amd.ops import kernels

DEV = "cpu"


# ------------------------------------------------------------ ts_bucket_agg
@pytest.mark.parametrize("name", list(ec.AGG_CASES))
def test_ts_bucket_agg(name):
    ec.check_agg(ec.run_agg(name, DEV), ec.agg_case(name)[2])


def test_agg_cases_have_their_shape():
    """The cases must really reach the branch they were built for."""
    def tile_ranges(name):
        chunks, args, _ = ec.agg_case(name)
        cells = ec.agg_cells(chunks[0], args)
        out = []
        for t0 in range(0, len(cells), ec.AGG_TILE):
            c = cells[t0:t0 + ec.AGG_TILE]
            c = c[c >= 0]
            assert len(c), "tile without a live row"
            out.append((int(c.min()), int(c.max() - c.min() + 1)))
        return out

    assert all(r > ec.LDS_CELLS for _, r in tile_ranges("unsorted_wide"))
    assert all(r <= ec.LDS_CELLS for n in (8191, 8192, 8193, 16385)
               for _, r in tile_ranges(f"sorted_{n}"))
    assert tile_ranges("lds_boundary")[:2] == [(7, 1024), (1031, 1025)]
    for name in ("floor_origin_pos", "floor_origin_neg"):
        chunks, args, exp = ec.agg_case(name)
        ts = chunks[0]["ts"]
        ts_lo, origin = args[0], args[2]
        assert ts_lo == origin - args[3] + 1
        assert ((ts >= ts_lo) & (ts < origin)).sum() > 50 and (ts < 0).any()
        assert exp["rows"][:, 0].sum() > 0
    _, _, exp = ec.agg_case("all_nan_cell")
    assert exp["rows"][2, 0] > 0 and exp["cnt"][1, 2, 0] == 0
    assert exp["sum"][1, 2, 0] == 0 and np.isnan(exp["min"][1, 2, 0])


def test_agg_extremes_exact_minmax():
    _, _, exp = ec.agg_case("extremes")
    assert exp["min"][0, :, 0].tolist() == [-1e308, -5e-324, 0.0]
    assert exp["max"][0, :, 0].tolist() == [1e308, 5e-324, 0.0]
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


def test_prom_case_has_its_shape():
    d = ec.prom_data()
    assert (d["hi"] - d["lo"]).tolist() == ec.PROM_SIZES
    # window t = 4 holds every sample of every segment
    exp, _ = ec.prom_expected(orc.COUNT, 0.0, False)
    full = np.where(np.isnan(exp[:, 4]), 0, exp[:, 4])
    assert full.tolist() == ec.PROM_SIZES
    # a sample on tb is out, a sample on te is in: segment 2 = [-3500, 1500]
    assert np.isnan(exp[2, 0]) and exp[2, 1] == 1 and exp[2, 3] == 2
    assert exp[2, 5] == 1                      # tb == -3500 excluded
    # all-NaN window: min/max NaN; NaN next to numbers: skipped
    mn, _ = ec.prom_expected(orc.MIN, 0.0, True)
    assert np.isnan(mn[2, 4]) and np.isfinite(mn[3, 4])


def test_prom_grid_stride_count_last():
    data, count, last = ec.prom_wide()
    assert len(data["lo"]) * ec.PROM_WIDE_GRID["T"] > ec.GRID_SPAN
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


def test_series_last_case_has_its_shape():
    sources, lut = ec.series_last_case()
    ts_u, src_u, _ = ec.series_last_expected(ec.UNBOUNDED)
    # ties go to the later source, whichever of the two is the sorted one
    assert (ts_u[3], src_u[3]) == (9000, 1) and (ts_u[4], src_u[4]) == (9500, 2)
    assert (ts_u[6], src_u[6]) == (9700, 2)
    assert src_u[12:].tolist() == [-1, -1, -1]
    assert min(int(t.min()) for t, _, _ in sources) < -4000
    # the bounded window cuts segment-last rows of sorted source 2 only
    lo, hi = ec.BOUNDED

    def cut(ts, series):
        last = {int(s): int(t) for t, s in zip(ts, series) if 0 <= s < 60}
        return any(not (lo <= t < hi) for t in last.values())

    assert not cut(*sources[0][:2]) and cut(*sources[2][:2])


# --------------------------------------------------------------- RLE expand
@pytest.mark.parametrize("bw", range(1, 33))
def test_rle_expand(bw):
    runs, blob, n, values = ec.rle_case(bw)
    np.testing.assert_array_equal(orc.rle_expand(runs, blob, bw, n), values)
    got = pagedec._expand_cpu(runs, blob, bw, n)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, values)


def test_rle_expand_one_long_run():
    runs, blob, n, values = ec.rle_case_big()
    probe = [0, 1, 7, 8, ec.GRID_SPAN - 1, ec.GRID_SPAN]
    np.testing.assert_array_equal(
        orc.rle_expand(runs, blob, 13, n, only=probe)[probe], values[probe])
    np.testing.assert_array_equal(pagedec._expand_cpu(runs, blob, 13, n),
                                  values)


# ------------------------------------------------------------------ gorilla
@pytest.mark.parametrize("ts_kind,val_kind,block,pack_ts", ec.GORILLA_CASES)
def test_gorilla_roundtrip(ts_kind, val_kind, block, pack_ts):
    ts, vals, packed = ec.gorilla_case(ts_kind, val_kind, block, pack_ts)
    hdr = ec.gorilla_headers(packed)
    assert sum(h[2] for h in hdr) == ec.GORILLA_N
    ts_bits = {h[0] for h in hdr if h[2] > 1}
    val_bits = {h[1] for h in hdr if h[2] > 1}
    if not pack_ts or ts_kind == "const":
        assert ts_bits == {0}
    if ts_kind == "minus1" and block % 2 == 0:
        assert ts_bits == {1}
    if ts_kind == "pm2_62":
        assert {63, 64} <= ts_bits
    if val_kind.startswith("const"):
        assert val_bits == {0}
    if val_kind.startswith("scaled_"):
        assert {h[3:] for h in hdr} == {(1, int(val_kind[-1]))}
    if val_kind in ("raw_special", "off_grid", "const_raw"):
        assert {h[3] for h in hdr} == {0}
    got_ts, got_vals = gorilla.decode_ref(*packed)
    ec.check_gorilla(ts, vals, packed, block, pack_ts,
                     got_ts.numpy(), got_vals.numpy())


@pytest.mark.parametrize("vals", [
    [0.1 + 0.2, 0.3, 1.0, 2.5, 0.7],
    [1.0, -0.0, 2.0],
    [0.1234, np.nextafter(0.1234, 1.0), 7.0],
    [1.5, float("nan"), float("inf"), -float("inf"), 5e-324, -2.2e-308],
])
def test_gorilla_keeps_every_bit(vals):
    """The codec is lossless: values near, but not on, the decimal grid and
    -0.0 must come back with the bits they went in with."""
    v = np.array(vals, dtype=np.float64)
    ts = np.arange(len(v), dtype=np.int64) * 1000
    _ts, got = gorilla.decode_ref(*gorilla.pack(ts, v))
    assert got.numpy().view(np.uint64).tolist() == v.view(np.uint64).tolist()


def test_gorilla_quantized_walk_still_compresses():
    """TSBS-shaped data (4 fixed decimals) must keep the scaled-int mode.
    Values clipped to [0, 100] at scale 10^4 differ by < 2^20 → zigzag deltas
    take <= 21 bits; ts deltas < 4095·20000 < 2^27 → <= 28 bits. 49 bits a row
    against 128 raw, header and padding included: better than 2.5×."""
    rng = np.random.RandomState(4)
    n = 50_000
    ts = 1451606400000 + np.cumsum(rng.randint(1, 20000, n)).astype(np.int64)
    v = np.round(np.clip(np.cumsum(rng.uniform(-1, 1, n)) + 50, 0, 100), 4)
    packed = gorilla.pack(ts, v)
    hdr = ec.gorilla_headers(packed)
    assert {h[3:] for h in hdr} == {(1, 4)}
    assert max(h[1] for h in hdr) <= 21 and max(h[0] for h in hdr) <= 28
    assert len(packed[0]) * 2.5 < 16 * n
    got_ts, got = gorilla.decode_ref(*packed)
    np.testing.assert_array_equal(got_ts.numpy(), ts)
    np.testing.assert_array_equal(got.numpy().view(np.uint64),
                                  v.view(np.uint64))


# ------------------------------------------------- filter / dedup / scatter
@pytest.mark.parametrize("n", ec.SMALL_SIZES)
@pytest.mark.parametrize("use_lut", [True, False])
def test_filter_series_time(n, use_lut):
    ts, series, lut = ec.rows_case(n)
    lut = lut if use_lut else None
    got = kernels.filter_series_time(
        torch.as_tensor(ts), torch.as_tensor(series),
        torch.as_tensor(lut) if use_lut else None, -20, 30)
    np.testing.assert_array_equal(
        got.numpy(), orc.filter_series_time(ts, series, lut, -20, 30))


@pytest.mark.parametrize("n", ec.SMALL_SIZES)
def test_dedup_mark_last(n):
    ts, series, _ = ec.rows_case(n)
    got = kernels.dedup_mark_last(torch.as_tensor(series), torch.as_tensor(ts))
    exp = orc.dedup_mark_last(series, ts)
    assert n < 2 or not exp.all()
    np.testing.assert_array_equal(got.numpy(), exp)


@pytest.mark.parametrize("n", (0, 1, 257))
@pytest.mark.parametrize("R", (1, 3))
def test_scatter_append(n, R):
    got, exp = ec.run_scatter(n, R, DEV)
    for g_list, e_list in zip(got, exp):
        for g, e in zip(g_list, e_list):
            np.testing.assert_array_equal(g, e)
