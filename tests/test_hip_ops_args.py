"""Argument checks of the _hip_ops bindings (csrc/hip_ops.cpp): an invalid
call raises RuntimeError before anything is queued, a valid one computes what
the CPU reference computes.

Every op is described once in OPS: a valid argument list of at most 8 rows
and the paths of its tensor arguments. The tests replace one tensor at a time.
Nothing here can touch memory out of bounds even if a check were missing: a
wrong-device tensor is pinned host memory (device-visible), a non-contiguous
tensor a strided view of a larger allocation, a too-short tensor a contiguous
prefix view of a full-length allocation, and blobs carry spare zero bytes.

The wrong-device test also runs without a GPU. There every tensor is on the
CPU, so all of an op's parametrisations make the same call and only the op's
FIRST check is exercised (it must be what raises, before anything else
happens). One check per tensor position is exercised only where there is a
GPU: the other tensors are then on the device and the one under test is
pinned host memory.
"""

import copy

import numpy as np
import pytest
import torch

import _edge_cases as ec
from greptimedb_amd.engine import gorilla, pagedec
from greptimedb_amd.ops import cpu_ref

H = pytest.importorskip("greptimedb_amd._hip_ops")

HAS_GPU = torch.cuda.is_available()
DEV = "cuda:0" if HAS_GPU else "cpu"

N, NF, N_SLOTS, N_BUCKETS = 8, 2, 2, 3
WINDOW = (0, 65)                      # ts_lo, ts_hi
BUCKETS = (0, 25)                     # origin, bucket_ms
TS = [10, 10, 20, 30, 40, 50, 60, 70]
SERIES = [0, 0, 1, 1, 2, 2, 3, 3]     # (series, ts)-sorted, one duplicate key
LUT = [0, 1, -1, 1]
# whole numbers: every sum is exact in any order
FIELDS = [[1, 2, 3, float("nan"), 5, 6, 7, 8], [-1, 0, 4, 9, 2, 2, 6, 3]]
REGION = [0, 1, 1, 0, 0, 1, 0, 1]
DST_OFF = [0, 0, 1, 1, 2, 2, 3, 3]
CAP = 6                               # rows per destination memtable


def _t(data, dtype):
    return torch.tensor(data, dtype=dtype, device=DEV)


def _rows():
    return (_t(TS, torch.int64), _t(SERIES, torch.int32),
            _t(LUT, torch.int32))


def _fields():
    return _t(FIELDS, torch.float64)


def _acc():
    """The accumulators ts_bucket_agg itself starts from."""
    shape = (NF, N_SLOTS, N_BUCKETS)
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)
    return [torch.zeros(shape, dtype=torch.float64, device=DEV), z(shape),
            torch.full(shape, -1, dtype=torch.int64, device=DEV), z(shape),
            z(shape[1:])]


def _agg_args(acc):
    ts, series, lut = _rows()
    return [ts, series, _fields(), _t([0, 1], torch.int32), lut, *WINDOW,
            *BUCKETS, N_SLOTS, N_BUCKETS, acc]


def _dests():
    return ([torch.full((CAP,), -7, dtype=torch.int64, device=DEV) for _ in "ab"],
            [torch.full((CAP,), -7, dtype=torch.int32, device=DEV) for _ in "ab"],
            [torch.full((NF, CAP), -7.0, dtype=torch.float64, device=DEV)
             for _ in "ab"])


def _scatter_args():
    ts, series, _ = _rows()
    return [ts, series, _fields(), _t(REGION, torch.int32),
            _t(DST_OFF, torch.int64), *_dests()]


def _packed_args():
    used = 8 * N + 8 * NF * N + 8 * N + 2 * ((4 * N + 7) & ~7)
    host = torch.zeros(used + 64, dtype=torch.uint8)
    seg = cpu_ref.packed_segments(host, N, NF)
    for dst, src in zip(seg, (TS, FIELDS, DST_OFF, SERIES, REGION)):
        dst.copy_(torch.tensor(src, dtype=dst.dtype))
    if HAS_GPU:
        host = host.pin_memory()
    return [host, torch.zeros(used + 64, dtype=torch.uint8, device=DEV), N, NF,
            [0, 0], *_dests()]


def _rle_case():
    runs, blob, n, _ = ec._rle_build(np.random.RandomState(5), 5,
                                     [(0, 3), (1, 5)])
    return runs, blob + b"\x00" * 64, n


def _rle_args():
    runs, blob, n = _rle_case()
    return [_t(runs.tolist(), torch.int64),
            _t(list(blob), torch.uint8), 5, n]


def _gorilla_case():
    return gorilla.pack(np.array(TS, dtype=np.int64),
                        np.array(FIELDS[1], dtype=np.float64), block=4)


def _gorilla_args():
    blob, block_off, out_off, n = _gorilla_case()
    return [_t(list(blob + b"\x00" * 64), torch.uint8),
            _t(block_off.tolist(), torch.int64),
            _t(out_off.tolist(), torch.int64), n]


def _prom_args():
    ts, _, _ = _rows()
    return [ts, _t(FIELDS[1], torch.float64), _t([0, 2, 4], torch.int64),
            _t([2, 4, 8], torch.int64), 4, 0, 25, 30, 0, 0.0,
            cpu_ref.PROM_MODES["last_over_time"]]


def _last_args(row):
    ts, series, lut = _rows()
    key = torch.zeros(N_SLOTS, dtype=torch.int64, device=DEV)
    args = [ts, series, lut, *WINDOW, key]
    if row:
        args += [3, torch.zeros(N_SLOTS, dtype=torch.int64, device=DEV)]
    return args


def _cells():
    ts, series, lut = _rows()
    return cpu_ref.bucket_cells(ts.cpu(), series.cpu(), lut.cpu(), *WINDOW,
                                *BUCKETS, N_BUCKETS).to(DEV)


# name -> (function, valid arguments, paths of the tensor arguments)
OPS = {
    "ts_bucket_agg": (H.ts_bucket_agg, lambda: _agg_args([]),
                      [(0,), (1,), (2,), (3,), (4,)]),
    "ts_bucket_agg_acc": (H.ts_bucket_agg, lambda: _agg_args(_acc()),
                          [(11, k) for k in range(5)]),
    "ts_bucket_agg_finish": (H.ts_bucket_agg_finish, lambda: [_acc()],
                             [(0, k) for k in range(5)]),
    "filter_series_time": (H.filter_series_time,
                           lambda: [*_rows(), *WINDOW], [(0,), (1,), (2,)]),
    "dedup_mark_last": (H.dedup_mark_last,
                        lambda: [_rows()[1], _rows()[0]], [(0,), (1,)]),
    "merge_last_non_null": (H.merge_last_non_null,
                            lambda: [_rows()[1], _rows()[0], _fields()],
                            [(0,), (1,), (2,)]),
    "series_last_ts": (H.series_last_ts, lambda: _last_args(False),
                       [(0,), (1,), (2,), (5,)]),
    "series_last_row": (H.series_last_row, lambda: _last_args(True),
                        [(0,), (1,), (2,), (5,), (7,)]),
    "prom_range_eval": (H.prom_range_eval, _prom_args,
                        [(0,), (1,), (2,), (3,)]),
    "scatter_append": (H.scatter_append, _scatter_args,
                       [(0,), (1,), (2,), (3,), (4,), (5, 1), (6, 1), (7, 1)]),
    "scatter_append_packed": (H.scatter_append_packed, _packed_args,
                              [(1,), (5, 1), (6, 1), (7, 1)]),
    "rle_expand_indices": (H.rle_expand_indices, _rle_args, [(0,), (1,)]),
    "gorilla_decode": (H.gorilla_decode, _gorilla_args, [(0,), (1,), (2,)]),
    "gorilla_encode": (H.gorilla_encode,
                       lambda: [_rows()[0], _t(FIELDS[1], torch.float64), 4,
                                True], [(0,), (1,)]),
    "bucket_cells": (H.bucket_cells,
                     lambda: [*_rows(), *WINDOW, *BUCKETS, N_BUCKETS],
                     [(0,), (1,), (2,)]),
    "grouped_quantile": (H.grouped_quantile,
                         lambda: [[[_cells(), _fields(),
                                    _t([0, 1], torch.int32)]], [0, 1],
                                  [0.5, 1.0], N_SLOTS * N_BUCKETS, None, 16],
                         [(0, 0, 0), (0, 0, 1), (0, 0, 2)]),
}
CASES = [(name, path) for name, (_, _, paths) in OPS.items() for path in paths]
IDS = [f"{name}-{'.'.join(map(str, path))}" for name, path in CASES]


def _get(args, path):
    for k in path:
        args = args[k]
    return args


def _with(args, path, value):
    """A copy of `args` with the tensor at `path` replaced."""
    out = copy.copy(args)
    if len(path) == 1:
        out[path[0]] = value
    else:
        out[path[0]] = _with(list(args[path[0]]), path[1:], value)
    return out


def _device_alive():
    torch.cuda.synchronize()
    assert int((torch.arange(10, device=DEV) * 2).sum().item()) == 90


def _prefix(t, shape):
    """Contiguous tensor of `shape` that is a prefix of t's own storage."""
    return t.reshape(-1)[:int(np.prod(shape))].view(shape)


def _raises(fn, args, match=None):
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


# ----------------------------------------------------------------- no GPU
def test_constants_match_edge_cases():
    assert (H.AGG_TILE, H.LDS_CELLS) == (ec.AGG_TILE, ec.LDS_CELLS)


@pytest.mark.parametrize("name,path", CASES, ids=IDS)
def test_wrong_device(name, path):
    fn, make, _ = OPS[name]
    args = make()
    if HAS_GPU:
        args = _with(args, path, _get(args, path).cpu().pin_memory())
    _raises(fn, args, match="must be a GPU tensor|pinned host memory")
    if HAS_GPU:
        _device_alive()


# ------------------------------------------------------------------- GPU
_OTHER = {torch.int64: torch.int32, torch.int32: torch.int64,
          torch.float64: torch.float32, torch.uint8: torch.int8}


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", CASES, ids=IDS)
def test_wrong_dtype(name, path):
    fn, make, _ = OPS[name]
    args = make()
    t = _get(args, path)
    _raises(fn, _with(args, path, t.to(_OTHER[t.dtype])))
    _device_alive()


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", CASES, ids=IDS)
def test_non_contiguous(name, path):
    fn, make, _ = OPS[name]
    args = make()
    t = _get(args, path)
    strided = t.repeat_interleave(2, dim=-1)[..., ::2]
    assert strided.shape == t.shape and not strided.is_contiguous()
    _raises(fn, _with(args, path, strided))
    _device_alive()


def _short(args, path):
    t = _get(args, path)
    return _with(args, path, t[:t.shape[0] - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", [
    ("filter_series_time", (1,)), ("dedup_mark_last", (0,)),
    ("series_last_ts", (1,)), ("series_last_row", (1,)),
    ("scatter_append", (1,)), ("scatter_append", (3,)),
    ("scatter_append", (4,)), ("prom_range_eval", (1,)),
    ("prom_range_eval", (3,)), ("gorilla_decode", (2,))])
def test_short_tensor(name, path):
    fn, make, _ = OPS[name]
    _raises(fn, _short(make(), path), match="length|one element per row")
    _device_alive()


@pytest.mark.gpu
def test_scatter_append_shapes():
    fn, make, _ = OPS["scatter_append"]
    args = make()
    _raises(fn, _with(args, (2,), _prefix(args[2], (NF, N - 1))), "nf, n")
    _raises(fn, _with(args, (2,), args[2].reshape(-1)), "nf, n")
    _raises(fn, _with(args, (6,), args[6][:1]), "lists differ")
    _raises(fn, _with(args, (7, 1), args[7][1][:NF - 1]), "fewer field rows")
    _device_alive()
    fn(*args)
    exp = [[x.cpu() for x in d] for d in _dests()]
    cpu = [a.cpu() for a in args[:5]]
    cpu_ref.scatter_append(*cpu, *exp)
    for got, want in zip(args[5:], exp):
        for g, w in zip(got, want):      # NaN == NaN here, the batch has one
            np.testing.assert_array_equal(g.cpu().numpy(), w.numpy())


@pytest.mark.gpu
def test_rle_expand_indices_shapes():
    fn, make, _ = OPS["rle_expand_indices"]
    args = make()
    runs = args[0]
    _raises(fn, _with(args, (0,), runs.reshape(-1)), "R, 5")
    _raises(fn, _with(args, (0,), _prefix(runs, (runs.shape[0], 4))), "R, 5")
    _raises(fn, _with(args, (0,), runs[:0]), "no runs")
    for bw in (0, 33):
        _raises(fn, args[:2] + [bw, args[3]], "bw must be in")
    _device_alive()
    r, blob, n = _rle_case()
    np.testing.assert_array_equal(fn(*args).cpu().numpy(),
                                  pagedec._expand_cpu(r, blob, 5, n))


@pytest.mark.gpu
def test_gorilla_decode_lengths():
    fn, make, _ = OPS["gorilla_decode"]
    args = make()
    _raises(fn, [args[0], args[1][:0], args[2][:0], args[3]], "no blocks")
    _device_alive()
    ts, vals = fn(*args)
    want_ts, want_vals = gorilla.decode_ref(*_gorilla_case())
    assert torch.equal(ts.cpu(), want_ts)
    assert torch.equal(vals.cpu().view(torch.int64), want_vals.view(torch.int64))


@pytest.mark.gpu
def test_ts_bucket_agg_acc_shape_and_range():
    fn = H.ts_bucket_agg
    args = _agg_args(_acc())
    small = (NF, N_SLOTS - 1, N_BUCKETS)
    # every accumulator a prefix of a full-size allocation
    shrunk = [_prefix(a, small if a.dim() == 3 else small[1:]) for a in _acc()]
    _raises(fn, _with(args, (11,), shrunk), "another nf, n_slots or n_buckets")
    _raises(fn, _with(args, (11, 4), _acc()[4].reshape(-1)), "acc must be four")
    _raises(fn, _with(args, (11,), _acc()[:4]), "5 raw accumulators")
    # cell ids are int32: the products must fit, whatever acc holds
    for n_slots, n_buckets in ((1 << 31, 1), (1 << 16, 1 << 16),
                               (1 << 15, 1 << 15)):
        big = list(args)
        big[9], big[10] = n_slots, n_buckets
        _raises(fn, big, "int32 cell arithmetic")
    _device_alive()
    got = H.ts_bucket_agg_finish(fn(*args))
    want = cpu_ref.ts_bucket_agg(*[a.cpu() for a in args[:5]], *args[5:11])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w.numpy())


@pytest.mark.gpu
def test_valid_calls_match_cpu_ref():
    ts, series, lut = (t.cpu() for t in _rows())
    a = OPS["filter_series_time"][1]()
    assert torch.equal(H.filter_series_time(*a).cpu(),
                       cpu_ref.filter_series_time(ts, series, lut, *WINDOW))
    a = OPS["dedup_mark_last"][1]()
    assert torch.equal(H.dedup_mark_last(*a).cpu(),
                       cpu_ref.dedup_mark_last(series, ts))
    a = _prom_args()
    np.testing.assert_array_equal(
        H.prom_range_eval(*a).cpu().numpy(),
        cpu_ref.prom_range_eval(*[x.cpu() for x in a[:4]], *a[4:]).numpy())
    # lastpoint: both raw passes against cpu_ref.series_last of one source
    a = _last_args(True)
    H.series_last_ts(*a[:6])
    H.series_last_row(*a)
    b_ts, b_src, b_row = cpu_ref.series_last([(ts, series)], lut, *WINDOW,
                                             N_SLOTS)
    found = b_src >= 0
    want_key = torch.where(found, b_ts ^ -(1 << 63), torch.zeros_like(b_ts))
    want_row = torch.where(found, (3 << 40) | (b_row + 1),
                           torch.zeros_like(b_row))
    assert found.all()
    assert torch.equal(a[5].cpu(), want_key)
    assert torch.equal(a[7].cpu(), want_row)


@pytest.mark.gpu
def test_lastpoint_empty_lut_hides_every_row():
    """An empty LUT has no series in it: nothing is visible, as in
    cpu_ref.series_last (only filter_series_time reads an empty LUT as "all
    series"). best_key / best_row have slots, so a kernel that took row 0's
    slot for granted would show here as a changed value, nothing more."""
    a = _last_args(True)
    a[2] = a[2][:0]
    H.series_last_ts(*a[:6])
    H.series_last_row(*a)
    torch.cuda.synchronize()
    assert not a[5].any() and not a[7].any()
    ts, series, _ = (t.cpu() for t in _rows())
    _, b_src, _ = cpu_ref.series_last(
        [(ts, series)], torch.zeros(0, dtype=torch.int32), *WINDOW, N_SLOTS)
    assert (b_src < 0).all()
