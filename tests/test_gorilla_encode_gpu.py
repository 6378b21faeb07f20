"""K20 encoder on the device (gorilla_{scale,widths,write}_kernel): the blob,
block_off and out_off must be byte for byte what gorilla.pack, the
specification, returns; and the engine's cold tier must stay in HBM. Every
comparison is against the host packer; no tolerance is involved. Runs on an
MI355X."""

import numpy as np
import pytest
import torch

import _edge_cases as ec
from greptimedb_amd import _hip_ops, ops
from greptimedb_amd.engine import gorilla
from greptimedb_amd.engine import sst as sst_mod

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _encode(ts, vals, block=gorilla.BLOCK, pack_ts=True):
    got = ops.gorilla_encode(_dev(ts), None if vals is None else _dev(vals),
                             block=block, pack_ts=pack_ts)
    assert all(t.is_cuda for t in got[:3])
    return got


def _assert_equals_pack(got, want):
    blob, block_off, out_off, n = got
    w_blob, w_block_off, w_out_off, w_n = want
    assert n == w_n
    assert blob.dtype == torch.uint8
    assert block_off.dtype == torch.int64 and out_off.dtype == torch.int64
    np.testing.assert_array_equal(block_off.cpu().numpy(), w_block_off)
    np.testing.assert_array_equal(out_off.cpu().numpy(), w_out_off)
    g = blob.cpu().numpy()
    w = np.frombuffer(w_blob, dtype=np.uint8)
    assert g.shape == w.shape
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (
        f"{bad.size} bytes differ, first at {bad[:8]}: "
        f"got {g[bad[:8]]}, want {w[bad[:8]]}")


# ------------------------------------------------------- edge-case parity
@pytest.mark.parametrize("ts_kind,val_kind,block,pack_ts", ec.GORILLA_CASES)
def test_edge_case_parity(ts_kind, val_kind, block, pack_ts):
    ts, vals, packed = ec.gorilla_case(ts_kind, val_kind, block, pack_ts)
    got = _encode(ts, vals, block, pack_ts)
    _assert_equals_pack(got, packed)
    # and the device blob feeds the existing device decoder as it is
    got_ts, got_vals = _hip_ops.gorilla_decode(got[0], got[1], got[2], got[3])
    ec.check_gorilla(ts, vals, packed, block, pack_ts,
                     got_ts.cpu().numpy(), got_vals.cpu().numpy())


# ------------------------------------------------------------ width sweep
def _width_sweep():
    """64 blocks of 67 values; block w-1 has ts zigzag deltas and XOR
    payloads of exactly w bits (w = 1..64). 66 packed values per block put
    (count-1)·w on and off byte and 8-byte boundaries."""
    rng = np.random.RandomState(20)
    block, k = 67, 66
    base_bits = np.array([0.1 + 0.2]).view(np.uint64)[0]
    ts_base = np.uint64(1700000000000)
    ts_parts, v_parts = [], []
    for w in range(1, 65):
        mask = np.uint64((1 << w) - 1)
        top = np.uint64(1 << (w - 1))

        def payload():
            p = (rng.randint(0, 1 << 32, k).astype(np.uint64) << np.uint64(32)
                 | rng.randint(0, 1 << 32, k).astype(np.uint64)) & mask
            p[0] |= top
            return p

        pv = payload()
        v_parts.append(np.concatenate([[base_bits], pv ^ base_bits]))
        zz = payload()
        d = (zz >> np.uint64(1)) ^ (np.uint64(0) - (zz & np.uint64(1)))
        ts_parts.append(np.concatenate([[ts_base], ts_base + d]))   # wraps
    ts = np.concatenate(ts_parts).astype(np.uint64).view(np.int64)
    vals = np.concatenate(v_parts).astype(np.uint64).view(np.float64)
    return ts, vals, block


def test_width_sweep_every_width_in_both_sections():
    ts, vals, block = _width_sweep()
    with np.errstate(all="ignore"):
        packed = gorilla.pack(ts, vals, block=block)
    hdr = ec.gorilla_headers(packed)
    assert [h[0] for h in hdr] == list(range(1, 65))
    assert [h[1] for h in hdr] == list(range(1, 65))
    assert all(h[2] == 67 and h[3] == 0 for h in hdr)
    got = _encode(ts, vals, block)
    _assert_equals_pack(got, packed)
    got_ts, got_vals = _hip_ops.gorilla_decode(got[0], got[1], got[2], got[3])
    ec.check_gorilla(ts, vals, packed, block, True,
                     got_ts.cpu().numpy(), got_vals.cpu().numpy())


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [0, 1, 2, 4095, 4096, 4097])
@pytest.mark.parametrize("with_vals", [True, False])
def test_sizes(n, with_vals):
    rng = np.random.RandomState(30 + n % 100)
    ts = (1451606400000 + np.cumsum(rng.randint(1, 20000, n))).astype(np.int64)
    vals = np.round(np.cumsum(rng.uniform(-1, 1, n)) + 50, 2) + 0.0
    if with_vals:
        _assert_equals_pack(_encode(ts, vals, 4096), gorilla.pack(ts, vals))
        _assert_equals_pack(_encode(ts, vals, 4096, pack_ts=False),
                            gorilla.pack(ts, vals, pack_ts=False))
    else:
        want = gorilla.pack(ts, np.zeros(n))
        _assert_equals_pack(_encode(ts, None, 4096), want)
        assert all(h[1] == 0 and h[3] == 1 and h[4] == 0
                   for h in ec.gorilla_headers(want))


# --------------------------------------------- mode selection, column-wide
def _modes(packed):
    return sorted({(h[3], h[4]) for h in ec.gorilla_headers(packed)})


def test_single_nan_in_last_block_makes_every_block_xor():
    rng = np.random.RandomState(40)
    n = 64 * 5 + 9
    ts = np.arange(n, dtype=np.int64) * 1000
    vals = np.round(rng.uniform(-500, 500, n), 2) + 0.0
    assert _modes(gorilla.pack(ts, vals, block=64)) == [(1, 2)]
    vals[-3] = np.nan
    want = gorilla.pack(ts, vals, block=64)
    assert _modes(want) == [(0, 0)]
    _assert_equals_pack(_encode(ts, vals, 64), want)


LIM = float(1 << 47)


@pytest.mark.parametrize("name,col,modes", [
    ("below_k0", [1.0, LIM - 1, -(LIM - 1), 7.0], [(1, 0)]),
    ("at_k0", [1.0, LIM - 1, LIM, 7.0], [(0, 0)]),
    ("neg_at_k0", [1.0, -LIM, 7.0], [(0, 0)]),
    # one decimal: fails k=0 on the round trip, then k=1 on the range
    ("below_k1", [0.5, (LIM - 8) / 10 - 0.5], [(1, 1)]),
    ("at_k1", [0.5, LIM / 10 + 0.5], [(0, 0)]),
    ("k3_not_k2", [1.25, -3.125, 0.001, 99.5], [(1, 3)]),
    ("k4", [1.25, 0.0001], [(1, 4)]),
    ("k5_is_xor", [1.25, 0.00001], [(0, 0)]),
    ("neg_zero", [1.0, -0.0, 2.0], [(0, 0)]),
    ("huge_finite", [1.0, 1.7e308], [(0, 0)]),
])
def test_mode_selection_matches_host(name, col, modes):
    reps = 50                       # several blocks of 64, last one partial
    vals = np.tile(np.asarray(col, dtype=np.float64), reps)
    ts = np.arange(len(vals), dtype=np.int64) * 10
    with np.errstate(all="ignore"):
        want = gorilla.pack(ts, vals, block=64)
    assert _modes(want) == modes
    _assert_equals_pack(_encode(ts, vals, 64), want)


def test_block_over_4096_raises():
    ts = _dev(np.arange(10, dtype=np.int64))
    vals = _dev(np.zeros(10))
    with pytest.raises(RuntimeError, match="block"):
        ops.gorilla_encode(ts, vals, block=4097)
    with pytest.raises(RuntimeError, match="block"):
        ops.gorilla_encode(ts, vals, block=0)
    _assert_equals_pack(ops.gorilla_encode(ts, vals, block=4096),
                        gorilla.pack(np.arange(10), np.zeros(10)))


# ----------------------------------------------------------------- engine
Q_ROWS = "SELECT hostname, ts, usage_user, usage_idle FROM cpu ORDER BY hostname, ts"
Q_AGG = ("SELECT hostname, count(*) c, avg(usage_user) a, max(usage_system) m"
         " FROM cpu GROUP BY hostname ORDER BY hostname")


def _small_table(eng):
    from greptimedb_amd.engine.ingest import Ingestor
    from greptimedb_amd.models.tsbs import CpuWorkload
    from greptimedb_amd.query.executor import Executor
    Ingestor(eng).ingest_lines(CpuWorkload(scale=3).next_batch(6000))
    eng.flush_all()
    return Executor(eng)


def _batches(eng):
    return [b for st in eng.tables.values() for r in st.regions
            for b in r.sst_cache.values()]


def _host_copy(b):
    return dict(ts=b.ts.cpu().numpy().copy(),
                fields=b.fields.cpu().numpy().copy(),
                series=b.series.cpu().numpy().copy(),
                seq=None if b.seq is None else b.seq.cpu().numpy().copy())


def _want_blobs(h):
    want = {"__ts": gorilla.pack(h["ts"], np.zeros(len(h["ts"])))[0]}
    for i in range(h["fields"].shape[0]):
        want[f"f{i}"] = gorilla.pack(h["ts"], h["fields"][i],
                                     pack_ts=False)[0]
    return want


def _blob_bytes(g):
    return g.blob.cpu().numpy().tobytes() if torch.is_tensor(g.blob) \
        else g.blob


def test_engine_compress_table_stays_on_device(gpu_engine):
    ex = _small_table(gpu_engine)
    batches = _batches(gpu_engine)
    assert batches and sum(b.n for b in batches) == 6000
    host = [_host_copy(b) for b in batches]
    rows, agg = ex.execute(Q_ROWS).rows(), ex.execute(Q_AGG).rows()
    assert len(rows) == 6000 and len(agg) == 3

    r = ex.execute("ADMIN compress_table('cpu')")
    bytes_before, bytes_after = int(r.columns[0][0]), int(r.columns[1][0])
    held = 0
    first = []
    for b, h in zip(batches, host):
        assert b.ts is None and b.fields is None and b.seq is None
        packs = {k: g for k, g in b._gorilla.items() if k != "__n"}
        want = _want_blobs(h)
        if h["seq"] is not None:
            want["__seq"] = gorilla.pack(h["seq"].astype(np.int64),
                                         np.zeros(len(h["seq"])))[0]
        assert sorted(packs) == sorted(want)
        for k, g in packs.items():
            assert g.blob.is_cuda and g.block_off.is_cuda and g.out_off.is_cuda
            assert _blob_bytes(g) == want[k], k
            held += g.nbytes
        # series never left the device, and no host copies were made
        assert torch.is_tensor(b.series) and b.series.is_cuda
        assert b._series_h is None and b._seq_h is None
        np.testing.assert_array_equal(b.series.cpu().numpy(), h["series"])
        held += b.n * 4
        first.append({k: _blob_bytes(g) for k, g in packs.items()})
    assert bytes_after == held
    assert 0 < bytes_after < bytes_before

    # scans re-materialize from the device blobs
    assert ex.execute(Q_ROWS).rows() == rows
    assert ex.execute(Q_AGG).rows() == agg
    for b, h in zip(batches, host):
        assert b.ts is not None and b.ts.is_cuda
        got = _host_copy(b)
        np.testing.assert_array_equal(got["ts"], h["ts"])
        np.testing.assert_array_equal(got["series"], h["series"])
        np.testing.assert_array_equal(got["fields"].view(np.uint64),
                                      h["fields"].view(np.uint64))
        if h["seq"] is not None:
            assert got["seq"].dtype == h["seq"].dtype
            np.testing.assert_array_equal(got["seq"], h["seq"])

    # compress → scan → compress again: the same bytes
    r2 = ex.execute("ADMIN compress_table('cpu')")
    assert int(r2.columns[1][0]) == bytes_after
    for b, f in zip(batches, first):
        again = {k: _blob_bytes(g) for k, g in b._gorilla.items()
                 if k != "__n"}
        assert again == f
    assert ex.execute(Q_AGG).rows() == agg


def test_engine_host_path_switch(gpu_engine, monkeypatch):
    monkeypatch.setattr(sst_mod.SstBatch, "_device_encode", False)
    ex = _small_table(gpu_engine)
    batches = _batches(gpu_engine)
    host = [_host_copy(b) for b in batches]
    rows, agg = ex.execute(Q_ROWS).rows(), ex.execute(Q_AGG).rows()
    r = ex.execute("ADMIN compress_table('cpu')")
    held = 0
    for b, h in zip(batches, host):
        packs = {k: g for k, g in b._gorilla.items() if k != "__n"}
        want = _want_blobs(h)
        assert sorted(packs) == sorted(want)
        for k, g in packs.items():
            assert isinstance(g.blob, bytes) and g.blob == want[k]
            held += g.nbytes
        assert b.series is None
        np.testing.assert_array_equal(b._series_h, h["series"])
        held += b.n * 4
    assert int(r.columns[1][0]) == held
    assert ex.execute(Q_ROWS).rows() == rows
    assert ex.execute(Q_AGG).rows() == agg
    assert all(b.ts is not None and b.ts.is_cuda for b in batches)


def test_compress_cold_takes_device_path(gpu_engine):
    ex = _small_table(gpu_engine)
    batches = _batches(gpu_engine)
    host = [_host_copy(b) for b in batches]
    agg = ex.execute(Q_AGG).rows()
    for b in batches:
        b.last_access = -1e9
    assert gpu_engine.compress_cold(age_s=1.0) == len(batches)
    for b, h in zip(batches, host):
        assert b.ts is None and b.series.is_cuda and b._series_h is None
        want = _want_blobs(h)
        for k, blob in want.items():
            g = b._gorilla[k]
            assert g.blob.is_cuda and _blob_bytes(g) == blob
    assert ex.execute(Q_AGG).rows() == agg
    assert all(b.ts is not None for b in batches)
